"""Griffin-Lim written with torch.linalg, torch.stft and torch.istft: the yardstick the Griffin-Lim kernels are tested and benchmarked
against (tests/test_griffinlim_*.py, tools/griffinlim_bench.py), for any float dtype and device.  Not a fallback: GriffinLimVocoder
never calls it.

It restates torchaudio's InverseMelScale (driver "gels") and GriffinLim(n_fft=1024, hop_length=256, power=2, momentum, rand_init)
as the reference configures them: magnitude(log-mel) -> S [513, T], then griffinlim(S, angles) -> waveform [256 (T - 1)].
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from kokoro_ruslan_amd.griffinlim import HOP, N_BINS, N_FFT, hann_window, inverse_mel_matrix, melscale_fbanks


def _complex(dtype: torch.dtype) -> torch.dtype:
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def magnitude(mel: torch.Tensor, dtype: torch.dtype = torch.float64, solver: str = "pinv") -> torch.Tensor:
    """S = relu(lstsq(fb^T, exp(mel)^T)) ^ (1/2), [513, T], for a log-mel [T, 80].  solver "pinv": the minimum-norm solution
    pinv(fb^T) . E (pinv in fp64, applied in dtype); "gels": torch.linalg.lstsq(driver="gels"), as the reference (CPU only)."""
    E = torch.exp(mel.to(dtype)).t()
    if solver == "gels":
        fbt = melscale_fbanks(torch.float64).t().to(dtype).to(mel.device)
        P = torch.linalg.lstsq(fbt[None], E[None], driver="gels").solution[0]
    else:
        P = inverse_mel_matrix().to(dtype).to(mel.device) @ E
    return torch.relu(P).pow(0.5)


def istft(Y: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    return torch.istft(Y, N_FFT, HOP, N_FFT, window)


def stft(x: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    return torch.stft(x, N_FFT, HOP, N_FFT, window, center=True, pad_mode="reflect", normalized=False, onesided=True,
                      return_complex=True)


def griffinlim(S: torch.Tensor, angles: Optional[torch.Tensor], n_iter: int = 60, momentum: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.griffinlim with power already applied: S [..., 513, T] magnitudes in the working dtype, angles the
    initial phases (None: ones).  Returns [..., 256 (T - 1)]."""
    dt = S.dtype
    window = hann_window(dt).to(S.device)
    angles = torch.ones(S.shape, dtype=_complex(dt), device=S.device) if angles is None else angles.to(_complex(dt)).to(S.device)
    beta = momentum / (1 + momentum)
    tprev = torch.zeros((), dtype=dt, device=S.device)
    for _ in range(n_iter):
        rebuilt = stft(istft(S * angles, window), window)
        angles = rebuilt - tprev * beta if momentum else rebuilt
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    return istft(S * angles, window)


def vocode(mel: torch.Tensor, angles: Optional[torch.Tensor] = None, n_iter: int = 60, momentum: float = 0.99,
           dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """One log-mel [T, 80] -> waveform [256 (T - 1)] in dtype, on mel's device (angles [513, T] or None: ones)."""
    return griffinlim(magnitude(mel, dtype), angles, n_iter, momentum)


def spectral_convergence(wave: torch.Tensor, S: torch.Tensor) -> float:
    """|| |STFT(wave)| - S || / ||S|| in fp64."""
    w = wave.double().to(S.device)
    R = stft(w, hann_window(torch.float64).to(S.device)).abs()
    S = S.double()
    return float((R - S).norm() / S.norm())


def harmonic_logmel(frames: int, seed: int = 0, f0: float = 120.0) -> torch.Tensor:
    """A speech-like test log-mel [frames, 80] (fp64, clamped to [-11.5, 2]): 29 harmonics of a vibrato around f0 with a 3 Hz
    envelope and a little noise, through the fp64 STFT and the mel filterbank."""
    from kokoro_ruslan_amd.griffinlim import SAMPLE_RATE
    g = torch.Generator().manual_seed(seed)
    n = HOP * (frames - 1)
    t = torch.arange(n, dtype=torch.float64) / SAMPLE_RATE
    pitch = f0 + 40.0 * torch.sin(2 * math.pi * 1.3 * t)
    ph = 2 * math.pi * torch.cumsum(pitch, 0) / SAMPLE_RATE
    x = sum(torch.sin(k * ph) / k for k in range(1, 30)) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t))
    x = x + 0.01 * torch.randn(n, dtype=torch.float64, generator=g)
    X = stft(x, hann_window(torch.float64))
    return torch.log(melscale_fbanks(torch.float64).t() @ X.abs() ** 2 + 1e-9).t().clamp(-11.5, 2.0).contiguous()


__all__ = ["magnitude", "istft", "stft", "griffinlim", "vocode", "spectral_convergence", "harmonic_logmel", "N_BINS"]
