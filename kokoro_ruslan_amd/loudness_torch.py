"""Edge trimming, ITU-R BS.1770-4 integrated loudness and loudness normalisation of mono waveforms in fp64 on the CPU: the yardstick
the loudness kernels are tested and benchmarked against (tests/test_loudness_*.py, tools/loudness_bench.py).  Not a fallback:
LoudnessNormaliser never calls it.

Edge trim: frame t covers samples [t hop - frame / 2, t hop + frame / 2), zeros outside the signal, T = 1 + n // hop frames,
rms_t = sqrt(sum x^2 / frame).  A frame is loud when 20 log10(rms_t / max rms) > -top_db.  With `first` and `last` the first and last
loud frames and m = round(margin_ms fs / 1000): start = max(0, first hop - m), end = min(n, (last + 1) hop + m).  An all-zero waveform
keeps [0, n).

Integrated loudness, one channel: the K-weighting is two biquads designed at fs from the analog prototypes (libebur128's constants;
at 48 kHz they are the standard's table), both from zero state at sample 0.  Blocks of N = round(0.4 fs) samples at step S =
round(0.1 fs), whole blocks only: nb = (n - N) // S + 1.  z_j = mean square of block j, l_j = -0.691 + 10 log10 z_j.  Absolute gate
l_j > -70; relative gate l_j > (-0.691 + 10 log10 mean(z over the absolute-gated blocks)) - 10; L = -0.691 + 10 log10 mean(z over the
blocks passing both).  No block, or none above the absolute gate: L = -inf.

Normalise: trim first if asked and measure the trimmed signal (filter state zero at `start`); g = 10^((target - L) / 20), lowered to
10^(peak_db / 20) / max|x[start:end]| where it would exceed that; L = -inf leaves g = 1.  The output is x[start:end] g.

trim_edges and integrated_loudness also return their decision margin: the smallest distance of any frame to the trim threshold (dB),
of any block to either gate (LU).  A test input whose margin is well above the device's error has the same decisions on the device.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

FRAME, HOP = 1024, 256
ABS_GATE, REL_GATE, OFFSET = -70.0, -10.0, -0.691
FS_MIN, FS_MAX = 8000, 48000


def block_sizes(fs: int) -> Tuple[int, int]:
    """(N, S): samples of a gating block and of its step."""
    return int(round(0.4 * fs)), int(round(0.1 * fs))


def kweight_coeffs(fs: float):
    """((b, a) of the shelving stage, (b, a) of the high-pass stage), a[0] = 1."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
          [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    s2 = ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return s1, s2


def biquad(x: torch.Tensor, b, a, chunk: int = 256) -> torch.Tensor:
    """y of the biquad (b, a) run over x [n] (fp64) from zero state.  Transposed direct form II, y_n = b0 x_n + s1, s1' = b1 x_n -
    a1 y_n + s2, s2' = b2 x_n - a2 y_n, i.e. s' = A s + c x_n with A = [[-a1, 1], [-a2, 0]], c = [b1 - a1 b0, b2 - a2 b0].  Run in
    chunks: the zero-state response of every chunk is one product with the chunk's impulse-response matrix, and only the two state
    values are carried from chunk to chunk in a loop."""
    n = int(x.numel())
    if n == 0:
        return x.clone()
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    C = int(chunk)
    A = torch.tensor([[-a1, 1.0], [-a2, 0.0]], dtype=torch.float64)
    c = torch.tensor([b1 - a1 * b0, b2 - a2 * b0], dtype=torch.float64)
    P = torch.empty(C + 1, 2, 2, dtype=torch.float64)           # A^k
    P[0] = torch.eye(2, dtype=torch.float64)
    for k in range(C):
        P[k + 1] = A @ P[k]
    h = torch.empty(C, dtype=torch.float64)                      # impulse response: h_0 = b0, h_k = (A^(k-1) c)[0]
    h[0] = b0
    h[1:] = (P[:C - 1] @ c)[:, 0]
    idx = torch.arange(C)
    lag = idx[:, None] - idx[None, :]
    H = torch.where(lag >= 0, h[lag.clamp(min=0)], torch.zeros((), dtype=torch.float64))      # y_i += h_(i-j) x_j
    Ys = P[:C, 0, :]                                             # y_i += (A^i s)[0]
    Sx = torch.flip(P[:C] @ c, dims=[0])                         # s' += A^(C-1-j) c x_j
    pad = (-n) % C
    X = torch.cat([x, x.new_zeros(pad)]).reshape(-1, C)
    Y = X @ H.T
    U = (X @ Sx).tolist()
    AC = P[C].tolist()
    s, states = (0.0, 0.0), []
    for u in U:
        states.append(s)
        s = (AC[0][0] * s[0] + AC[0][1] * s[1] + u[0], AC[1][0] * s[0] + AC[1][1] * s[1] + u[1])
    Y = Y + torch.tensor(states, dtype=torch.float64) @ Ys.T
    return Y.reshape(-1)[:n]


def kweight(x: torch.Tensor, fs: float) -> torch.Tensor:
    """The K-weighted signal [n] in fp64, both filters from zero state at sample 0."""
    (b1, a1), (b2, a2) = kweight_coeffs(fs)
    return biquad(biquad(_wave(x), b1, a1), b2, a2)


def _wave(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 1:
        raise ValueError(f"waveform of shape {tuple(x.shape)}: expected [samples]")
    return x.detach().to("cpu", torch.float64)


def _lufs(z: float) -> float:
    return OFFSET + 10.0 * math.log10(z) if z > 0 else -math.inf


def trim_edges(x: torch.Tensor, top_db: float = 40.0, margin_ms: float = 50.0, frame: int = FRAME, hop: int = HOP,
               fs: int = 22050) -> Tuple[int, int, float]:
    """(start, end, decision margin in dB)."""
    x = _wave(x)
    n = int(x.numel())
    xp = torch.cat([x.new_zeros(frame // 2), x, x.new_zeros(frame // 2)])
    rms = torch.sqrt((xp.unfold(0, frame, hop) ** 2).sum(dim=1) / frame)          # 1 + n // hop frames
    top = float(rms.max()) if n else 0.0
    if top == 0.0:
        return 0, n, math.inf
    db = 20.0 * torch.log10(rms / top)                            # -inf on a frame of zeros
    loud = torch.nonzero(db > -float(top_db)).reshape(-1)
    first, last = int(loud[0]), int(loud[-1])
    m = int(round(float(margin_ms) * fs / 1000.0))
    return max(0, first * hop - m), min(n, (last + 1) * hop + m), float((db + float(top_db)).abs().min())


def integrated_loudness(x: torch.Tensor, fs: int = 22050) -> Tuple[float, float]:
    """(L in LUFS or -inf, decision margin in LU)."""
    y = kweight(x, fs)
    n = int(y.numel())
    N, S = block_sizes(fs)
    if n < N:
        return -math.inf, math.inf
    z = (y.unfold(0, N, S) ** 2).mean(dim=1)                      # (n - N) // S + 1 blocks
    l = OFFSET + 10.0 * torch.log10(z)
    above = l > ABS_GATE
    if not bool(above.any()):
        return -math.inf, float((l - ABS_GATE).abs().min())
    rel = _lufs(float(z[above].mean())) + REL_GATE
    keep = above & (l > rel)
    margin = min(float((l - ABS_GATE).abs().min()), float((l - rel).abs().min()))
    return _lufs(float(z[keep].mean())), margin


def normalise(x: torch.Tensor, target_lufs: float = -23.0, peak_db: float = -1.0, trim: Optional[float] = None, fs: int = 22050,
              margin_ms: float = 50.0) -> Tuple[torch.Tensor, Dict]:
    """(x[start:end] g in fp64, {"start", "end", "measured" (None for -inf), "gain", "limited", "trim_margin", "gate_margin"})."""
    x = _wave(x)
    start, end, tm = (0, int(x.numel()), math.inf) if trim is None else trim_edges(x, trim, margin_ms, fs=fs)
    seg = x[start:end]
    L, gm = integrated_loudness(seg, fs)
    g, limited = 1.0, False
    if L > -math.inf:
        g = 10.0 ** ((float(target_lufs) - L) / 20.0)
        peak, ceiling = float(seg.abs().max()), 10.0 ** (float(peak_db) / 20.0)
        if g * peak > ceiling:
            g, limited = ceiling / peak, True
    return seg * g, {"start": start, "end": end, "measured": L if L > -math.inf else None, "gain": g, "limited": limited,
                     "trim_margin": tm, "gate_margin": gm}


__all__ = ["trim_edges", "integrated_loudness", "normalise", "kweight", "kweight_coeffs", "biquad", "block_sizes", "FRAME", "HOP",
           "FS_MIN", "FS_MAX"]
