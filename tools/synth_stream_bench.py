#!/usr/bin/env python3
"""Continuous batching against fixed batches: KokoroEngine.generate_stream at 8 / 32 / 64 slots against generate_batch on
consecutive groups of the same size, over the same utterances in the same order.  Default model size, random weights, 256 utterances
of 20-100 phonemes.  The stop head is out of play: the duration predictor's last layer is set to predict 3 frames per phoneme
(60-300 frames, a range of 5), and with stop_threshold = 0 and min_len_ratio = 1 each row ends right behind its own predicted
length.  Five repeats, the two paths interleaved inside every repeat (same process, same clocks, same weights); prints per slot
count the median wall time of each path, their spread, frames per second and the ratio, then one JSON line.

    python tools/synth_stream_bench.py [mode=bf16] [utterances=256] [repeats=5]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.spec import ModelDims, StepHyper

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SLOT_FRAMES = 512
KW = dict(max_len=SLOT_FRAMES, stop_threshold=0.0, min_len_ratio=1.0, min_len_floor=1)
g = torch.Generator().manual_seed(0)
utts = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (N,), generator=g)]

e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=0)
DP = "duration_adaptor.variance_adaptor.duration_predictor.linear"
e.arena.P[DP + ".weight"].zero_()                              # log-duration = the bias alone: round(expm1(1.4)) = 3 frames per phoneme
e.arena.P[DP + ".bias"].fill_(1.4)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def batches(S):
    out = []
    for i in range(0, N, S):
        out += e.generate_batch(utts[i:i + S], **KW)
    return out


def stream(S):
    return e.generate_stream(utts, slots=S, slot_frames=SLOT_FRAMES, **KW)


result = {"mode": mode, "utterances": N, "repeats": REPEATS, "slots": {}}
for S in (8, 32, 64):                                          # warm-up: workspaces at their final sizes, kernel attributes
    a, b = batches(S), stream(S)
    assert all(x.shape == y.shape for x, y in zip(a, b)), "the two paths must decode the same frame counts"
    frames = sum(m.shape[0] for m in a)
    lens = [m.shape[0] for m in a]
    result["slots"][S] = {"frames": frames, "batch_s": [], "stream_s": [],
                          "live_share": frames / sum(max(lens[i:i + S]) * len(lens[i:i + S]) for i in range(0, N, S))}
for _ in range(REPEATS):
    for S in (8, 32, 64):
        result["slots"][S]["batch_s"].append(timed(lambda: batches(S))[1])
        result["slots"][S]["stream_s"].append(timed(lambda: stream(S))[1])
print(f"{mode}: {N} utterances, {result['slots'][8]['frames']} frames, rows of {min(lens)}-{max(lens)} frames, {REPEATS} interleaved repeats")
for S, r in result["slots"].items():
    tb, ts = statistics.median(r["batch_s"]), statistics.median(r["stream_s"])
    r.update(batch_median_s=tb, stream_median_s=ts, speedup=tb / ts)
    print(f"  {S:2d} slots: generate_batch {tb * 1e3:8.1f} ms [{min(r['batch_s']) * 1e3:.1f}, {max(r['batch_s']) * 1e3:.1f}] = {r['frames'] / tb:8.0f} frames/s | "
          f"generate_stream {ts * 1e3:8.1f} ms [{min(r['stream_s']) * 1e3:.1f}, {max(r['stream_s']) * 1e3:.1f}] = {r['frames'] / ts:8.0f} frames/s | "
          f"x{tb / ts:.2f} (live share of a fixed batch's row-steps {r['live_share']:.2f})")
print(json.dumps(result))
