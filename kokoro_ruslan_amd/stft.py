"""The constants and host tables of the project's one STFT: 22050 Hz, n_fft = win = 1024, hop 256, 513 bins, 80 mels, periodic Hann.

The kernels of csrc/kk_fft.h take the window and the twiddle table from here; feature extraction (features.py), Griffin-Lim
(griffinlim.py) and spectral denoising (denoise.py) all build them through `device_tables`.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

SAMPLE_RATE, N_FFT, HOP, N_MELS = 22050, 1024, 256, 80
N_BINS = N_FFT // 2 + 1


def hann_window(dtype: torch.dtype = torch.float64) -> torch.Tensor:
    return torch.hann_window(N_FFT, periodic=True, dtype=dtype)


ANALYSIS_WIDTHS = (256, 512, 1024)      # the windows of the multi-resolution spectral distance (spectral.py); 1024 is hann_window


def centred_hann_windows(dtype: torch.dtype = torch.float64, widths=ANALYSIS_WIDTHS) -> torch.Tensor:
    """[len(widths), 1024]: a periodic Hann of each width w centred in the 1024-sample frame (entries 512 - w / 2 .. 512 + w / 2 - 1,
    zeros elsewhere): what torch.stft(n_fft=1024, win_length=w) makes of hann_window(w), so one 1024-point transform serves them all."""
    out = torch.zeros(len(widths), N_FFT, dtype=dtype)
    for r, w in enumerate(widths):
        if w % 2 or not (2 <= w <= N_FFT):
            raise ValueError(f"window width {w}: expected an even number in 2..{N_FFT}")
        out[r, N_FFT // 2 - w // 2:N_FFT // 2 + w // 2] = torch.hann_window(w, periodic=True, dtype=dtype)
    return out


def twiddles() -> torch.Tensor:
    """exp(-2 pi i j / 1024) for j < 1024, computed in fp64, as complex64."""
    ang = -2.0 * math.pi * torch.arange(N_FFT, dtype=torch.float64) / N_FFT
    return torch.polar(torch.ones_like(ang), ang).to(torch.complex64)


def device_tables(device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(window fp32 [1024], twiddles fp32 [1024, 2]) on the device, both rounded once from fp64."""
    return (hann_window(torch.float64).to(torch.float32).to(device), torch.view_as_real(twiddles()).contiguous().to(device))
