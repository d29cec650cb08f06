#!/usr/bin/env python3
"""Batched synthesis throughput: KokoroEngine.generate at B = 1 against generate_batch at B = 1, 8, 32, 64 (ragged phoneme counts),
default model size, random weights, stop head disabled (every row runs to its own length bound), fp32 parity mode and bf16 mode.
Prints mel frames per second of wall time (encode included) and ms per decode step.

    python tools/synth_bench.py [max_len=300]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.spec import ModelDims, StepHyper

max_len = int(sys.argv[1]) if len(sys.argv) > 1 else 300
KW = dict(max_len=max_len, stop_threshold=2.0, post_expected_stop_threshold=2.0)
g = torch.Generator().manual_seed(0)
pool = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (64,), generator=g)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


for mode in ("f32", "bf16"):
    e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=0)
    one = pool[0]
    e.generate(one[None], **dict(KW, max_len=20))                                     # warm-up: workspaces, kernel attributes
    mel, dt = timed(lambda: e.generate(one[None], **KW))
    n = mel.shape[1]
    print(f"{mode} generate       B=1 : {n:6d} frames in {dt * 1e3:8.1f} ms = {n / dt:8.0f} frames/s, {dt / n * 1e3:.3f} ms/step")
    for B in (1, 8, 32, 64):
        utts = pool[:B]
        e.generate_batch(utts, **dict(KW, max_len=20))
        mels, dt = timed(lambda: e.generate_batch(utts, **KW))
        n, steps = sum(m.shape[0] for m in mels), max(m.shape[0] for m in mels)
        ok = all(bool(torch.isfinite(m).all()) for m in mels)
        print(f"{mode} generate_batch B={B:<2d}: {n:6d} frames in {dt * 1e3:8.1f} ms = {n / dt:8.0f} frames/s, "
              f"{dt / steps * 1e3:.3f} ms/step ({steps} steps), finite={ok}")
