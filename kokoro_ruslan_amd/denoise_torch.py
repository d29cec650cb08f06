"""Spectral denoising written with torch.stft and torch.istft in fp64 on the CPU: the yardstick the denoising kernels are tested and
benchmarked against (tests/test_denoise_*.py, tools/denoise_bench.py).  Not a fallback: SpectralDenoiser never calls it.

The method, with the Griffin-Lim constants (n_fft = win = 1024, hop 256, periodic Hann, 513 bins, center with reflect padding): for a
waveform x of N >= 1024 samples, a bias b [513] >= 0 and a strength s >= 0,

    X = stft(x)  (1 + N // 256 frames);  M = |X|;  G = max(1 - s b[k] / M, 0), 0 where M = 0;  y = istft(G X, length = N)

which is max(M - s b, 0) with the phase kept, written so that it is continuous in M.  The bias of a vocoder is the mean of |stft| of
what it makes of a silent mel, over the frames whose window lies wholly inside the waveform (frames 2 .. F - 3).
"""
from __future__ import annotations

import torch

from kokoro_ruslan_amd.griffinlim import HOP, N_BINS, N_FFT, hann_window
from kokoro_ruslan_amd.griffinlim_torch import stft

MIN_SAMPLES = N_FFT


def _wave(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 1 or x.numel() < MIN_SAMPLES:
        raise ValueError(f"waveform of shape {tuple(x.shape)}: expected [samples >= {MIN_SAMPLES}]")
    return x.detach().to("cpu", torch.float64)


def gain(M: torch.Tensor, bias: torch.Tensor, strength: float) -> torch.Tensor:
    """G [513, F] for magnitudes M [513, F]."""
    t = float(strength) * bias.detach().to("cpu", torch.float64).reshape(N_BINS, 1)
    safe = torch.where(M > 0, M, torch.ones_like(M))
    return torch.where(M > 0, torch.clamp(1.0 - t / safe, min=0.0), torch.zeros_like(M))


def denoise(x: torch.Tensor, bias: torch.Tensor, strength: float) -> torch.Tensor:
    """The denoised waveform [N] in fp64."""
    x = _wave(x)
    w = hann_window(torch.float64)
    X = stft(x, w)
    return torch.istft(gain(X.abs(), bias, strength) * X, N_FFT, HOP, N_FFT, w, length=x.numel())


def bias_frames(n: int) -> range:
    """The frames whose window lies wholly inside a waveform of n samples: 2 .. F - 3 of its F = 1 + n // 256."""
    return range(2, 1 + n // HOP - 2)


def bias_from_wave(w: torch.Tensor) -> torch.Tensor:
    """[513] fp64: |stft(w)| averaged over bias_frames."""
    w = _wave(w)
    fr = bias_frames(w.numel())                      # never empty: 1024 samples make 5 frames
    return stft(w, hann_window(torch.float64)).abs()[:, fr.start:fr.stop].mean(dim=1)


__all__ = ["denoise", "gain", "bias_from_wave", "bias_frames", "MIN_SAMPLES"]
