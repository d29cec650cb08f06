"""The spectral distance of two waveforms along a DTW path, restated in fp64 on the CPU: the definition of the metric and the yardstick
kk_dtw_spectral_stats is tested and benchmarked against (tests/test_spectral_*.py, tools/spectral_bench.py).  Not a fallback:
SpectralDistance never calls it.

A pair is a, the synthesized waveform (n_a samples, vocoded from a mel of Ta frames), b, the recording (n_b samples, its cache mel has
Tb frames), and a path of steps (i_k, j_k) in mel frames.  Both waveforms are scaled as the feature extractor scales audio
(features_torch.normalise: x / (max|x| + 1e-9)).  Frame i is centred on sample 256 i with reflect padding by index, n_fft = 1024, 513
bins; three analysis windows, a periodic Hann of width 256, 512 and 1024 centred in the frame (stft.centred_hann_windows).  A step is
skipped, and counted as such, when i is outside [0, Ta), j outside [0, Tb), or a frame centre lies past its waveform (256 i > n_a or
256 j > n_b).  With A = |STFT_w(a)|[i], B = |STFT_w(b)|[j] at a counted step and d = 10 log10((A^2 + 1e-9) / (B^2 + 1e-9)) (the
log-mel's floor), five sums per window over all counted steps and bins: sum A B, sum A^2, sum B^2, sum d, sum d^2.  From them, with
N = counted steps x 513:

    sc_dtw[w]   = sqrt(max(0, 1 - (sum AB)^2 / (sum A^2 sum B^2)))   spectral convergence at the least-squares gain: a level
                                                                     difference costs nothing; None when a side is all zero
    level_db[w] = sum d / N                                          how much louder, in dB, the synthesized spectrum sits
    lsd_dtw[w]  = sqrt(max(0, sum d^2 / N - (sum d / N)^2))          log-spectral distance in dB, the level offset taken out

and mr_sc_dtw, mr_lsd_dtw: the means over the three windows.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from kokoro_ruslan_amd.features_torch import normalise
from kokoro_ruslan_amd.stft import ANALYSIS_WIDTHS, HOP, N_BINS, N_FFT, centred_hann_windows

WINDOWS = ANALYSIS_WIDTHS
SUMS = ("ab", "aa", "bb", "d", "dd")                     # the rows of a window, in the kernel's order
FLOOR = 1e-9
MIN_SAMPLES = N_FFT
MAX_STEPS = 8191                                         # Ta + Tb - 1 of the longest pair the DP takes
PER_WINDOW = ("sc_dtw", "lsd_dtw", "level_db")
FIELDS = tuple(f"{k}_{w}" for w in WINDOWS for k in PER_WINDOW) + ("mr_sc_dtw", "mr_lsd_dtw")
COUNTS = ("spec_steps", "spec_skipped")


def _wave(x: torch.Tensor) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.numel() < MIN_SAMPLES:
        raise ValueError(f"waveform of shape {tuple(getattr(x, 'shape', ()))}: expected [samples >= {MIN_SAMPLES}]")
    return normalise(x.detach().to("cpu"), torch.float64)


def magnitudes(x: torch.Tensor) -> torch.Tensor:
    """[3, 1 + n // 256, 513] fp64: |STFT_w| of an already scaled waveform, frame t centred on sample 256 t."""
    pad = F.pad(x[None], (N_FFT // 2, N_FFT // 2), mode="reflect")[0]
    frames = pad.unfold(0, N_FFT, HOP)
    return torch.fft.rfft(frames[None] * centred_hann_windows(torch.float64)[:, None, :], dim=-1).abs()


def spectral_stats(a: torch.Tensor, b: torch.Tensor, path, Ta: int, Tb: int) -> Dict[str, object]:
    """{"sums": fp64 [3, 5] (window x SUMS), "steps": counted steps, "skipped": skipped steps} of one pair."""
    a, b = _wave(a), _wave(b)
    path = torch.as_tensor(path).to("cpu", torch.int64).reshape(-1, 2)
    if path.shape[0] > MAX_STEPS:
        raise ValueError(f"a path of {path.shape[0]} steps; at most {MAX_STEPS}")
    i, j = path[:, 0], path[:, 1]
    ok = (i >= 0) & (i < int(Ta)) & (j >= 0) & (j < int(Tb)) & (HOP * i <= a.numel()) & (HOP * j <= b.numel())
    i, j = i[ok], j[ok]
    A, B = magnitudes(a)[:, i], magnitudes(b)[:, j]                   # [3, counted, 513]
    d = 10.0 * torch.log10((A * A + FLOOR) / (B * B + FLOOR))
    sums = torch.stack([(A * B).sum((1, 2)), (A * A).sum((1, 2)), (B * B).sum((1, 2)), d.sum((1, 2)), (d * d).sum((1, 2))], 1)
    return {"sums": sums, "steps": int(ok.sum()), "skipped": int((~ok).sum())}


def spectral_metrics(sums, steps: int, skipped: int = 0) -> Dict[str, object]:
    """The record fields of one pair from its fifteen sums ([3, 5] or a flat sequence of 15, window-major) and its counts."""
    s = [float(v) for v in torch.as_tensor(sums, dtype=torch.float64).reshape(-1).tolist()]
    if len(s) != 5 * len(WINDOWS):
        raise ValueError(f"{len(s)} sums; expected {5 * len(WINDOWS)}")
    out: Dict[str, object] = {}
    N = int(steps) * N_BINS
    sc: Sequence[Optional[float]] = []
    lsd: Sequence[Optional[float]] = []
    for r, w in enumerate(WINDOWS):
        ab, aa, bb, d, dd = s[5 * r:5 * r + 5]
        c = math.sqrt(max(0.0, 1.0 - (ab * ab) / (aa * bb))) if N and aa * bb > 0.0 else None
        mean = d / N if N else None
        l = math.sqrt(max(0.0, dd / N - mean * mean)) if N else None
        out[f"sc_dtw_{w}"], out[f"lsd_dtw_{w}"], out[f"level_db_{w}"] = c, l, mean
        sc.append(c)
        lsd.append(l)
    out["mr_sc_dtw"] = sum(sc) / len(sc) if all(v is not None for v in sc) else None
    out["mr_lsd_dtw"] = sum(lsd) / len(lsd) if all(v is not None for v in lsd) else None
    out["spec_steps"], out["spec_skipped"] = int(steps), int(skipped)
    return out


def measure(a: torch.Tensor, b: torch.Tensor, path, Ta: int, Tb: int) -> Dict[str, object]:
    st = spectral_stats(a, b, path, Ta, Tb)
    return spectral_metrics(st["sums"], st["steps"], st["skipped"])


__all__ = ["WINDOWS", "SUMS", "FIELDS", "COUNTS", "PER_WINDOW", "MIN_SAMPLES", "MAX_STEPS", "magnitudes", "spectral_stats", "spectral_metrics",
           "measure"]
