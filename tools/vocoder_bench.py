#!/usr/bin/env python3
"""HiFi-GAN vocoder throughput: HifiganVocoder.vocode on B = 1, 8, 32, 64 mels of 300 frames, default V1 config, random weights, in
both math modes, against the same generator written with torch.nn.functional conv1d / conv_transpose1d (vocoder_torch.forward on a
[B, 300, 80] batch) in fp32 and bf16.  Prints mel frames per second and the achieved TFLOP/s (2 x the generator's MACs as counted
from the config; the polyphase form's zero taps not counted).

    python tools/vocoder_bench.py [frames=300] [iters=5]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import vocoder_torch as VT
from kokoro_ruslan_amd.vocoder import DEFAULT_CONFIG, HifiganVocoder

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def macs_per_frame(cfg) -> float:
    c, m = cfg["upsample_initial_channel"], 80 * 7 * cfg["upsample_initial_channel"]
    rows = 1
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        m += rows * c * (c // 2) * k                                   # ConvTranspose1d: every input sample meets every tap
        rows, c = rows * u, c // 2
        m += rows * sum(2 * len(ds) * c * c * rk for rk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
    return m + rows * c * 7


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


cfg = dict(DEFAULT_CONFIG)
flop = 2 * macs_per_frame(cfg)
print(f"V1 generator: {flop / 1e9:.3f} GFLOP per mel frame, {frames}-frame mels, {iters} timed calls each")
sd = VT.random_state_dict(cfg, seed=0)
g = torch.Generator().manual_seed(0)
pool = [(torch.randn(frames, 80, generator=g) - 5.0).cuda() for _ in range(64)]
res = {}
for mode in ("bf16", "f32"):
    voc = HifiganVocoder(cfg, math_mode=mode)
    voc.load_state_dict(sd)
    for B in (1, 8, 32, 64):
        dt = timed(lambda: voc.vocode(pool[:B]))
        res[(mode, B)] = B * frames / dt
        print(f"kernels {mode:4s} B={B:<2d}: {dt * 1e3:9.2f} ms  {B * frames / dt:9.0f} frames/s  {B * frames * flop / dt / 1e12:7.2f} TFLOP/s")
    del voc
    torch.cuda.empty_cache()
base = HifiganVocoder(cfg, device="cpu", math_mode="f32")
base.load_state_dict(sd)
for mode, dtp in (("bf16", torch.bfloat16), ("f32", torch.float32)):
    W = {n: w.to("cuda", dtp) for n, w in base.weights.items()}
    Bi = {n: b.to("cuda", dtp) for n, b in base.biases.items()}
    for B in (1, 8, 32, 64):
        batch = torch.stack(pool[:B])
        with torch.no_grad():
            dt = timed(lambda: VT.forward(W, Bi, cfg, batch))
        r = B * frames / dt
        print(f"torch   {mode:4s} B={B:<2d}: {dt * 1e3:9.2f} ms  {r:9.0f} frames/s  {B * frames * flop / dt / 1e12:7.2f} TFLOP/s   "
              f"kernels / torch = {res[(mode, B)] / r:.2f}x")
