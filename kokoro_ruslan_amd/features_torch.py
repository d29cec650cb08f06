"""The audio feature extraction written with torch.stft / torch.fft: the yardstick the feature kernels are tested and benchmarked
against (tests/test_features_*.py, tools/features_bench.py), for any float dtype and device.  Not a fallback: FeatureExtractor never
calls it.

It restates what the reference's dataset computes per utterance (data/dataset.py:644-869, model/variance_predictor.py:442-688) at its
TrainingConfig defaults: the peak-normalised waveform, torchaudio's MelSpectrogram(power=2, Hann, center, reflect, HTK, norm=None) as
log(fb^T . |STFT|^2 + 1e-9), EnergyExtractor.extract_energy_from_mel(log_domain=False) and PitchExtractor.extract_pitch.  torchaudio is
not a dependency: the mel is pinned to its definition through griffinlim.melscale_fbanks (the one statement of the filterbank in this
repository) and torch.stft.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from kokoro_ruslan_amd.griffinlim import HOP, N_FFT, N_MELS, SAMPLE_RATE, hann_window, melscale_fbanks

PITCH_WIN, PITCH_FMIN, PITCH_FMAX = 2048, 50.0, 800.0
LAG_MIN, LAG_MAX = int(SAMPLE_RATE / PITCH_FMAX), int(SAMPLE_RATE / PITCH_FMIN)        # 27, 441
CMND_THRESHOLD, MAX_GAP, MEDIAN_K = 0.15, 5, 5


def mel_frames(n: int) -> int:
    return 1 + max(int(n), N_FFT) // HOP


def pitch_frames(n: int) -> int:
    return 1 + max(int(n), PITCH_WIN) // HOP


def normalise(wave: torch.Tensor, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """x / (max|x| + 1e-9), zero-padded to 1024 samples (dataset.py:672, :688-690)."""
    x = wave.to(dtype)
    x = x / (x.abs().max() + 1e-9)
    return F.pad(x, (0, N_FFT - x.shape[0])) if x.shape[0] < N_FFT else x


def mel_linear(x: torch.Tensor) -> torch.Tensor:
    """fb^T . |STFT(x)|^2, [80, 1 + n // 256], for a normalised waveform x in its dtype."""
    X = torch.stft(x, N_FFT, HOP, N_FFT, hann_window(x.dtype).to(x.device), center=True, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True)
    return melscale_fbanks(torch.float64).to(x.dtype).to(x.device).t() @ (X.real ** 2 + X.imag ** 2)


def energy(mel_lin: torch.Tensor) -> torch.Tensor:
    """EnergyExtractor.extract_energy_from_mel(mel_lin.T, log_domain=False) for a linear mel [80, T]."""
    e = torch.log1p(mel_lin.mean(0).clamp(min=0.0))
    if e.shape[0] < 3:
        lo, hi = e.min(), e.max()
    else:
        lo, hi = torch.quantile(e, 0.05), torch.quantile(e, 0.95)
    return ((e - lo) / torch.clamp(hi - lo, min=1e-8)).clamp(0.0, 1.0)


def pitch_candidates(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per pitch frame of a normalised waveform: the candidate frequency in Hz, the largest normalised autocorrelation over lags
    27..441 and the windowed frame's mean square: PitchExtractor.extract_pitch up to (not including) the voicing decision."""
    dt, dev = x.dtype, x.device
    if x.shape[0] < PITCH_WIN:
        x = F.pad(x, (0, PITCH_WIN - x.shape[0]))
    x = torch.cat([x[:1], x[1:] - 0.97 * x[:-1]])
    x = F.pad(x[None], (PITCH_WIN // 2, PITCH_WIN // 2), mode="reflect")[0]
    frames = x.unfold(0, PITCH_WIN, HOP) * torch.hann_window(PITCH_WIN, dtype=dt, device=dev)
    spec = torch.fft.rfft(frames, n=2 * PITCH_WIN)
    acf = torch.fft.irfft(spec.abs() ** 2, n=2 * PITCH_WIN)[..., :PITCH_WIN]
    r0 = acf[..., :1]
    diff = 2 * r0 - 2 * acf
    cmnd = torch.zeros_like(diff)
    cmnd[..., 0] = 1.0
    tau = torch.arange(1, PITCH_WIN, device=dev, dtype=dt)
    cmnd[..., 1:] = diff[..., 1:] / (torch.cumsum(diff[..., 1:], -1) / tau + 1e-8)
    c = cmnd[..., LAG_MIN:LAG_MAX + 1]
    n_lags = c.shape[-1]
    ac_max = (acf / r0.clamp(min=1e-8))[..., LAG_MIN:LAG_MAX + 1].max(-1).values
    below = c < CMND_THRESHOLD
    first = ((below.cumsum(-1) == 1) & below).long().argmax(-1)
    best = torch.where(below.any(-1), first, torch.argmin(c, -1))
    pick = lambda i: c.gather(-1, i[..., None])[..., 0]
    al, be, ga = pick((best - 1).clamp(min=0)), pick(best), pick((best + 1).clamp(max=n_lags - 1))
    off = (0.5 * (al - ga) / (al - 2 * be + ga).clamp(min=1e-8)).clamp(-1.0, 1.0)
    lag = ((best + LAG_MIN).float() + off).clamp(min=1.0)
    return SAMPLE_RATE / lag, ac_max, frames.pow(2).mean(-1)


def pitch_finish(freqs: torch.Tensor, ac_max: torch.Tensor, msq: torch.Tensor) -> torch.Tensor:
    """Voicing over the utterance's statistics, gap fill, median filter, normalisation: the rest of extract_pitch."""
    vth = torch.clamp(torch.quantile(ac_max, 0.25) * 0.8, min=0.15, max=0.35)
    eth = torch.clamp(torch.median(msq) * 0.05, min=1e-9)
    f = freqs.masked_fill((ac_max < vth) | (msq < eth), 0.0)
    f = torch.where((f < PITCH_FMIN) | (f > PITCH_FMAX), torch.zeros_like(f), f)
    T = f.shape[0]
    idx = torch.arange(T, device=f.device)
    voiced = f > 0.0
    if voiced.any():
        prev = torch.cummax(torch.where(voiced, idx, torch.full_like(idx, -1)), 0)[0]
        nxt = torch.cummin(torch.where(voiced, idx, torch.full_like(idx, T)).flip(0), 0)[0].flip(0)
        fill = (~voiced) & (prev >= 0) & (nxt < T) & (nxt - prev - 1 <= MAX_GAP)
        if fill.any():
            pv, nv = f[prev.clamp(min=0)], f[nxt.clamp(max=T - 1)]
            t = (idx.float() - prev.float()) / (nxt.float() - prev.float()).clamp(min=1.0)
            f = torch.where(fill, pv * (1.0 - t) + nv * t, f)
    pad = MEDIAN_K // 2
    f = F.pad(f[None], (pad, pad), mode="reflect")[0].unfold(0, MEDIAN_K, 1).median(-1).values
    out = torch.clamp((f - PITCH_FMIN) / (PITCH_FMAX - PITCH_FMIN + 1e-8), 0.0, 1.0)
    return out.masked_fill(f == 0.0, 0.0)


def pitch(x: torch.Tensor) -> torch.Tensor:
    """PitchExtractor.extract_pitch(x, 22050, 256, 50, 800) for a normalised waveform: [1 + max(n, 2048) // 256] in [0, 1]."""
    return pitch_finish(*pitch_candidates(x))


def extract(wave: torch.Tensor, max_seq_length: int = 1800, variance: bool = True,
            dtype: torch.dtype = torch.float64) -> Dict[str, object]:
    """One waveform (un-normalised mono samples) -> {"mel_spec" [80, T], "mel_linear" [80, T], "pitch" [T], "energy" [T],
    "mel_length" T} in dtype on wave's device, T = min(1 + max(n, 1024) // 256, max_seq_length)."""
    x = normalise(wave, dtype)
    lin = mel_linear(x)[:, :max_seq_length]
    T = lin.shape[1]
    out = {"mel_spec": torch.log(lin + 1e-9), "mel_linear": lin, "mel_length": T}
    if variance:
        p = pitch(x)[:T]
        out["pitch"] = torch.cat([p, p.new_zeros(T - p.shape[0])])
        out["energy"] = energy(lin)
    else:
        out["pitch"], out["energy"] = lin.new_zeros(T), lin.new_zeros(T)
    return out


def test_signal(n: int, seed: int = 0, f0: float = 120.0) -> torch.Tensor:
    """A speech-like test waveform of n samples (fp64, peak below 1): harmonic_logmel's source, 29 harmonics of a vibrato around f0 with
    a 3 Hz envelope, in a cycle of 0.22 s segments — voiced, voiced at a lower level, noise only, near silence — over a noise floor of 0.003."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SAMPLE_RATE
    f = f0 * (1.0 + 0.04 * torch.sin(2 * math.pi * 4.5 * t))
    ph = 2 * math.pi * torch.cumsum(f, 0) / SAMPLE_RATE
    harm = sum(torch.sin(k * ph) / k for k in range(1, 30)) / 2.0 * (0.6 + 0.4 * torch.sin(2 * math.pi * 3.0 * t))
    seg = (torch.arange(n) // int(0.22 * SAMPLE_RATE)) % 4
    level = torch.tensor([0.8, 0.45, 0.0, 0.0], dtype=torch.float64)[seg]
    noise = torch.tensor([0.0, 0.0, 0.08, 0.0], dtype=torch.float64)[seg]
    r = torch.randn(2, n, dtype=torch.float64, generator=g)
    return harm * level + noise * r[0] + 0.003 * r[1]


test_signal.__test__ = False            # a generator of test inputs, not a test

__all__ = ["normalise", "mel_linear", "energy", "pitch_candidates", "pitch_finish", "pitch", "extract", "test_signal", "mel_frames",
           "pitch_frames"]
