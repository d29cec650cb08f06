#!/usr/bin/env python3
"""Spectral-denoising throughput: SpectralDenoiser.denoise on B = 1, 8, 32, 64 waveforms of 300 x 256 samples at the default strength,
against the same method written with torch.stft / torch.istft in fp32 on the same GPU on a [B, samples] batch.  Five repeats, the two
interleaved per batch size; prints the medians (ms per call, samples per second) and the ratio.

    python tools/denoise_bench.py [frames=300] [iters=20]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd.denoise import DEFAULT_STRENGTH, SpectralDenoiser
from kokoro_ruslan_amd.griffinlim import HOP, N_BINS, N_FFT

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 20
REPEATS = 5
n = frames * HOP


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


g = torch.Generator().manual_seed(0)
pool = [(0.1 * torch.randn(n, generator=g)).cuda() for _ in range(64)]
den = SpectralDenoiser()
den.set_bias(0.05 * (1.0 + torch.cos(torch.arange(N_BINS, dtype=torch.float64) / 20.0)))
window = den.window
sb = (DEFAULT_STRENGTH * den.bias)[None, :, None]


def torch_gpu(x):
    X = torch.stft(x, N_FFT, HOP, N_FFT, window, center=True, pad_mode="reflect", return_complex=True)
    M = X.abs()
    G = torch.where(M > 0, torch.clamp(1.0 - sb / M.clamp(min=1e-30), min=0.0), torch.zeros_like(M))
    return torch.istft(G * X, N_FFT, HOP, N_FFT, window, length=x.shape[1])


print(f"spectral denoising, {frames} x {HOP}-sample waveforms, {iters} timed calls per repeat, medians of {REPEATS} interleaved repeats")
for B in (1, 8, 32, 64):
    waves, stacked = pool[:B], torch.stack(pool[:B])
    a = float((den.denoise(waves)[0] - torch_gpu(stacked)[0]).norm() / torch_gpu(stacked)[0].norm())
    ours, theirs = [], []
    for _ in range(REPEATS):
        ours.append(timed(lambda: den.denoise(waves)))
        theirs.append(timed(lambda: torch_gpu(stacked)))
    do, dt = statistics.median(ours), statistics.median(theirs)
    print(f"B={B:<2d}: kernels {do * 1e3:8.3f} ms  {B * n / do / 1e6:9.1f} M samples/s   torch GPU {dt * 1e3:8.3f} ms  "
          f"{B * n / dt / 1e6:9.1f} M samples/s   kernels / torch GPU = {dt / do:.2f}x   (rel L2 between them {a:.1e})")
