#!/usr/bin/env python3
"""Throughput of the DTW kernels and their share of a free-running evaluation.

Part 1: MelAligner.run_packed (cepstra, DP, backtrack, sums along the path: everything an alignment costs on the device) at B = 1, 8,
32, 64 pairs of 300 x 300 and of 1600 x 1800 frames, against two baselines: the fp64 oracle (kokoro_ruslan_amd.dtw_torch) on the host
in 16 threads, and an anti-diagonal DTW written with torch ops on the same GPU (the DP alone, all pairs of the batch per op, no path).
Five repeats with the device paths interleaved inside every repeat; medians, with the spread.  The host oracle runs once per size
on 16 pairs (it takes seconds).
Part 2: evaluate() at 32 slots on the utterance mix of tools/synth_stream_bench.py (256 utterances of 20-100 phonemes, 3 frames per
phoneme, random weights), against ground truths of 0.9-1.1 times the synthesized length: the time of the synthesis, of the alignment,
and the alignment's share of the call.  One JSON line at the end.

    python tools/dtw_bench.py [mode=bf16] [utterances=256] [repeats=5]"""
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import dtw_torch as R
from kokoro_ruslan_amd.dtw import MelAligner

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SIZES, BATCHES, M = ((300, 300), (1600, 1800)), (1, 8, 32, 64), 80
al = MelAligner()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def pairs(B, Ta, Tb, seed):
    g = torch.Generator().manual_seed(seed)
    syn = [(torch.randn(Ta, M, generator=g) * 2 - 5).cuda() for _ in range(B)]
    ref = [(s[torch.linspace(0, Ta - 1, Tb).round().long().cuda()] + 0.1 * torch.randn(Tb, M, generator=g).cuda()) for s in syn]
    return syn, ref


def torch_dtw(ca, cb):
    """D(Ta-1, Tb-1) [B] of cepstra [B, Ta, K], [B, Tb, K] with torch ops, one anti-diagonal of every pair at a time."""
    B, Ta, Tb = ca.shape[0], ca.shape[1], cb.shape[1]
    d = torch.zeros(B, Ta, Tb, device=ca.device)
    for k in range(ca.shape[2]):
        d += (ca[:, :, None, k] - cb[:, None, :, k]) ** 2
    d = d.sqrt()
    D = torch.full((B, Ta + 1, Tb + 1), float("inf"), device=d.device)
    D[:, 1, 1] = d[:, 0, 0]
    rows = torch.arange(Ta, device=d.device)
    for s in range(1, Ta + Tb - 1):
        i = rows[max(0, s - Tb + 1):min(s, Ta - 1) + 1]
        j = s - i
        D[:, i + 1, j + 1] = d[:, i, j] + torch.minimum(torch.minimum(D[:, i, j], D[:, i, j + 1]), D[:, i + 1, j])
    return D[:, Ta, Tb]


result = {"mode": mode, "repeats": REPEATS, "dtw": {}, "evaluate": {}}
cases = {}
for Ta, Tb in SIZES:
    for B in BATCHES:
        syn, ref = pairs(B, Ta, Tb, 1000 * B + Ta)
        run = al.run_packed(syn, ref)                           # warm-up, and the cepstra for the baselines
        ca = run["ca"].t().reshape(B, Ta, -1).contiguous()
        cb = run["cb"].t().reshape(B, Tb, -1).contiguous()
        ours, base = run["total"].cpu(), torch_dtw(ca, cb).cpu()
        gap = float(((ours - base).abs() / base).max())         # the two device paths must find the same optimum, up to fp32 summation
        print(f"{Ta} x {Tb}, B = {B}: kernels against torch ops, largest relative difference of the totals {gap:.2e}"
              + ("" if gap <= (Ta + Tb + 32) * 2.0 ** -22 else "  <-- MORE than two fp32 sums of Ta + Tb terms explain"))
        cases[(Ta, Tb, B)] = (syn, ref, ca, cb, {"kernel_s": [], "torch_s": [], "totals_rel_gap": gap})
for _ in range(REPEATS):
    for key, (syn, ref, ca, cb, r) in cases.items():
        r["kernel_s"].append(timed(lambda: al.run_packed(syn, ref))[1])
        r["torch_s"].append(timed(lambda: torch_dtw(ca, cb))[1])
torch.set_num_threads(1)                                        # 16 pairs side by side, one thread each
for Ta, Tb in SIZES:
    syn, ref, ca, cb, _ = cases[(Ta, Tb, 64)]
    ca, cb = ca[:16].cpu().numpy(), cb[:16].cpu().numpy()
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda n: R.dtw(ca[n], cb[n])[0], range(16)))
        host = time.perf_counter() - t0
    result["dtw"][f"{Ta}x{Tb}"] = {"host_oracle_16_threads_pairs_per_s": 16 / host}
    print(f"{Ta} x {Tb}: fp64 oracle on the host, 16 pairs in 16 threads: {host:.2f} s = {16 / host:.1f} pairs/s = {16 * Ta * Tb / host / 1e6:.1f} M cells/s")
    for B in BATCHES:
        r = cases[(Ta, Tb, B)][4]
        tk, tt = statistics.median(r["kernel_s"]), statistics.median(r["torch_s"])
        r.update(kernel_median_s=tk, torch_median_s=tt, pairs_per_s=B / tk, cells_per_s=B * Ta * Tb / tk)
        result["dtw"][f"{Ta}x{Tb}"][B] = r
        print(f"  B = {B:2d}: kernels {tk * 1e3:8.2f} ms [{min(r['kernel_s']) * 1e3:.2f}, {max(r['kernel_s']) * 1e3:.2f}] = {B / tk:8.0f} pairs/s = "
              f"{B * Ta * Tb / tk / 1e9:6.2f} G cells/s | torch ops (DP only) {tt * 1e3:8.1f} ms [{min(r['torch_s']) * 1e3:.1f}, {max(r['torch_s']) * 1e3:.1f}] | x{tt / tk:.0f}")

# ---- part 2: the alignment's share of an evaluate() call ------------------------------------------------------------------------
from kokoro.inference.evaluate import evaluate
from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.spec import ModelDims, StepHyper

SLOT_FRAMES = 512
KW = dict(max_len=SLOT_FRAMES, stop_threshold=0.0, min_len_ratio=1.0, min_len_floor=1, slot_frames=SLOT_FRAMES)
g = torch.Generator().manual_seed(0)
utts = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (N,), generator=g)]
e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=0)
DP = "duration_adaptor.variance_adaptor.duration_predictor.linear"
e.arena.P[DP + ".weight"].zero_()                              # log-duration = the bias alone: 3 frames per phoneme
e.arena.P[DP + ".bias"].fill_(1.4)
mels = e.generate_stream(utts, slots=32, **KW)                 # warm-up
refs = [torch.randn(max(1, int(m.shape[0] * float(torch.empty(1).uniform_(0.9, 1.1, generator=g)))), m.shape[1], generator=g).cuda() * 2 - 5
        for m in mels]
evaluate(e, utts, None, refs, slots=32, aligner=al, **KW)
ev = {"synth_s": [], "align_s": [], "evaluate_s": []}
for _ in range(REPEATS):
    mels, t = timed(lambda: e.generate_stream(utts, slots=32, want_info=True, **KW)[0])
    ev["synth_s"].append(t)
    ev["align_s"].append(timed(lambda: al.align(mels, refs))[1])
    ev["evaluate_s"].append(timed(lambda: evaluate(e, utts, None, refs, slots=32, aligner=al, **KW))[1])
frames = sum(m.shape[0] for m in mels)
ts, ta, te = (statistics.median(ev[k]) for k in ("synth_s", "align_s", "evaluate_s"))
ev.update(utterances=N, frames=frames, synth_median_s=ts, align_median_s=ta, evaluate_median_s=te, align_share=ta / te)
result["evaluate"] = ev
print(f"evaluate, {mode}, 32 slots: {N} utterances, {frames} frames: synthesis {ts * 1e3:.1f} ms [{min(ev['synth_s']) * 1e3:.1f}, {max(ev['synth_s']) * 1e3:.1f}] "
      f"= {frames / ts:.0f} frames/s | alignment {ta * 1e3:.1f} ms [{min(ev['align_s']) * 1e3:.1f}, {max(ev['align_s']) * 1e3:.1f}] | "
      f"evaluate {te * 1e3:.1f} ms | the alignment's share {100 * ta / te:.1f} %")
print(json.dumps(result))
