"""The resampler's contract in torch: torchaudio's `sinc_interp_hann` (lowpass_filter_width 6, rolloff 0.99), the method behind
`torchaudio.functional.resample` at its defaults, which the reference calls for its speed perturbation (data/dataset.py:674-684) and
for corpora at another rate (:662-665).  What csrc/kk_resample.hip is tested against.

With the rates reduced by their gcd to o (in) and n (out), base = 0.99 min(o, n), width = ceil(6 o / base) and L' = ceil(n L / o),
output sample j = q n + p (0 <= p < n) is

    y[j] = sum over m = c - width .. c + width, c = floor(p o / n), of x[q o + m] h(t),      x = 0 outside [0, L)
    t    = base (m n - p o) / (o n) clamped to [-6, 6],   h(t) = (base / o) sinc(pi t) cos(pi t / 12)^2,   sinc(0) = 1

torchaudio builds h for every phase p as an [n, 1, 2 width + o] kernel over m in [-width, width + o) and convolves with stride o; the
clamp puts every tap with |t| >= 6 on the window's zero, and the 2 width + 1 taps above hold every other one.  `resample` never builds
that kernel (1.85 GB for 22050 -> 20947): it is vectorised over the outputs and loops over the taps.

`order="integer"` (the default) forms the phase numerator m n - p o in integers and scales it once: exact in fp64, the oracle.
`order="torchaudio"` reproduces torchaudio's own operation order, t = (-p / n + m / o) base with every step in `dtype`; in fp32 the
two quotients round separately and t carries an error of ~1e-7 o, which for coprime rates near 22050 is 4e-4 of the signal.  It is
kept for the record (DESIGN §5 "Resampling"), not as a reference.  torchaudio itself is not needed and not imported.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def rate_pair(orig_freq: int, new_freq: int) -> Tuple[int, int, float, int]:
    """(o, n, base, width) of a rate pair: the rates reduced by their gcd, 0.99 min(o, n), ceil(6 o / base)."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"sample rates must be positive integers, not {orig_freq!r} -> {new_freq!r}")
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * ROLLOFF
    return o, n, base, int(math.ceil(LOWPASS_FILTER_WIDTH * o / base))


def resampled_length(length: int, orig_freq: int, new_freq: int) -> int:
    """ceil(n L / o), in integers."""
    o, n, _, _ = rate_pair(orig_freq, new_freq)
    return (n * int(length) + o - 1) // o


def resample(x: torch.Tensor, orig_freq: int, new_freq: int, dtype: torch.dtype = torch.float64, order: str = "integer") -> torch.Tensor:
    """x [L] -> [ceil(n L / o)] in `dtype` (taps and sums).  Equal rates return x unchanged, as torchaudio does."""
    if order not in ("integer", "torchaudio"):
        raise ValueError(f"order must be 'integer' or 'torchaudio', not {order!r}")
    if x.dim() != 1:
        raise ValueError(f"expected a 1-D waveform, got shape {tuple(x.shape)}")
    if int(orig_freq) == int(new_freq):
        return x
    o, n, base, width = rate_pair(orig_freq, new_freq)
    L = x.shape[0]
    xd = x.to(dtype)
    j = torch.arange(resampled_length(L, orig_freq, new_freq), dtype=torch.int64, device=x.device)
    q, p = j // n, j % n
    c = (p * o) // n
    y = torch.zeros(j.shape[0], dtype=dtype, device=x.device)
    zero = torch.zeros((), dtype=dtype, device=x.device)
    # torchaudio's kernel spans m in [-width, width + o); one tap more on each side than the definition shows that they carry nothing
    taps = range(-width, width + 1) if order == "integer" else range(-width - 1, width + 2)
    for d in taps:
        m = c + d
        if order == "integer":
            t = (m * n - p * o).to(dtype) * torch.tensor(base / (o * n), dtype=torch.float64).to(dtype)
            inside = torch.ones_like(m, dtype=torch.bool)
        else:
            t = ((-p).to(dtype) / n + m.to(dtype) / o) * base
            inside = (m >= -width) & (m < width + o)
        t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
        window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
        t = t * math.pi
        h = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)
        i = q * o + m
        ok = inside & (i >= 0) & (i < L)
        y += torch.where(ok, xd[i.clamp(0, max(L - 1, 0))], zero) * h
    return y


def peak_normalise(x: torch.Tensor) -> torch.Tensor:
    """audio / (max |audio| + 1e-9) (dataset.py:672, :684)."""
    return x / (x.abs().max() + 1e-9)


def speed_perturb(x: torch.Tensor, factor: float, sample_rate: int = 22050, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """dataset.py:672-684: normalise, resample sample_rate -> int(sample_rate factor), normalise."""
    y = resample(peak_normalise(x.to(dtype)), sample_rate, int(sample_rate * factor), dtype)
    return peak_normalise(y.to(dtype))
