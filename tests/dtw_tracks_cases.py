"""Inputs shared by the track-metric device tests (test_dtw_tracks_kernels_gpu.py, test_evaluate_audio_gpu.py)."""
import torch


def pitch_track(g: torch.Generator, n: int, unvoiced: float = 0.4) -> torch.Tensor:
    """A normalised pitch track of n frames: runs of 1-9 frames, each unvoiced (0) with probability `unvoiced`, else 80-380 Hz."""
    p = 0.04 + 0.4 * torch.rand(n, generator=g)
    i = 0
    while i < n:
        L = int(torch.randint(1, 10, (1,), generator=g))
        if float(torch.rand(1, generator=g)) < unvoiced:
            p[i:i + L] = 0.0
        i += L
    return p


def close(got: float, want: float) -> bool:
    """The bound of the kernel's fp64 sums against the oracle's on the same path and tracks: 1e-9 relative, 1e-9 absolute near zero
    (fp64 log2 within a few ulp, at most 8191 steps: about 4e-12; three orders of margin)."""
    return abs(got - want) <= max(1e-9 * abs(want), 1e-9)
