#!/usr/bin/env python3
"""Cost of the pronunciation scores (kk_align_scores) beside the alignment they ride on.

64 utterances of 300 tokens x 1800 frames and 64 of 100 x 600.  Per size, on the L, label and durations of one run_packed(): the two
launches of PhoneAligner.score_packed; the same sums written with torch ops on the same GPU (max / argmax over the classes, the fp64
log-sum-exp, gathers by label and segment sums by token: what one would write without the kernel); the Viterbi launch alone on the same
L, the launch the scores are expected to stay far below; and a whole PhoneAligner.score call, of which the share of the new launches is
reported.  Five repeats with the paths interleaved inside every repeat; medians, with the spread.  One JSON line at the end.

    python tools/align_scores_bench.py [repeats=5]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.align import PhoneAligner

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SIZES, B, M, V = ((300, 1800), (100, 600)), 64, 80, 59
al = PhoneAligner(n_classes=V)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def corpus(n, P, T, seed):
    """n utterances whose frames follow their tokens' class templates in an uneven split (tools/align_bench.py's)."""
    g = torch.Generator().manual_seed(seed)
    templates = torch.randn(V, M, generator=g) * 2.0 - 5.0
    mels, ids = [], []
    for _ in range(n):
        i = torch.randint(0, V, (P,), generator=g)
        d = torch.ones(P, dtype=torch.long) + torch.bincount(torch.randint(0, P, (T - P,), generator=g), minlength=P)
        mels.append((templates[torch.repeat_interleave(i, d)] + 0.5 * torch.randn(T, M, generator=g)).cuda())
        ids.append(i)
    return mels, ids


def torch_scores(run):
    """(gop_sum, lpost_sum, hits per token; the three totals per utterance) with torch ops.  The segment sums are index_add_: their
    order is not the kernel's, so the values agree to rounding, not bit for bit."""
    L, label, dur = run["L"], run["label"].long(), run["durations"].long()
    P_total, Bn = dur.shape[0], len(run["foff_host"]) - 1
    fmax, amax = L.max(0)
    Ld = L.double()
    lse = (Ld - fmax.double()).exp().sum(0).log()
    margin = Ld.gather(0, label.clamp(min=0)[None])[0] - fmax.double()
    lpost = margin - lse
    token = torch.repeat_interleave(torch.arange(P_total, device=L.device), dur)          # (every utterance feasible here)
    gop = torch.zeros(P_total, dtype=torch.float64, device=L.device).index_add_(0, token, margin)
    lp = torch.zeros(P_total, dtype=torch.float64, device=L.device).index_add_(0, token, lpost)
    hits = torch.zeros(P_total, dtype=torch.int64, device=L.device).index_add_(0, token, (amax == label).long())
    utt = torch.repeat_interleave(torch.arange(Bn, device=L.device), (run["poff"][1:] - run["poff"][:-1]).long())
    tot = [torch.zeros(Bn, dtype=x.dtype, device=L.device).index_add_(0, utt, x) for x in (gop, lp, hits)]
    return gop, lp, hits, tot


def viterbi_launch(run, pk_threads, opt, coff):
    kk.call("kk_align_viterbi", run["L"], run["L"].shape[1], run["ids"], opt, run["foff"], run["poff"], coff, B, pk_threads, 1,
            run["score"], run["end"], run["codes"])


result = {"repeats": REPEATS, "sizes": {}}
cases = {}
for P, T in SIZES:
    mels, ids = corpus(B, P, T, 1000 + P)
    model, _, _ = al.fit(mels, ids, iters=2)                    # warm-up, and a model worth scoring with
    run = al.run_packed(mels, ids, (), model)
    sc, ref = al.score_packed(run), torch_scores(run)
    assert bool((run["score"] > float("-inf")).all())
    assert torch.equal(sc["hits"].long(), ref[2]), "the torch restatement counts other hits"
    gap = float(((sc["gop_sum"] - ref[0]).abs().max() / ref[0].abs().max()).cpu())
    lgap = float(((sc["lpost_sum"] - ref[1]).abs().max() / ref[1].abs().max()).cpu())
    print(f"{P} x {T}: kernels against torch ops, largest difference of gop_sum {gap:.2e}, of lpost_sum {lgap:.2e} (relative to the largest sum)")
    opt = torch.zeros(B * P, dtype=torch.uint8, device="cuda")
    coff = torch.tensor(run["coff_host"], dtype=torch.int64).cuda()
    al.score(mels, ids, (), model)
    cases[(P, T)] = (mels, ids, model, run, opt, coff, {"scores_s": [], "torch_s": [], "viterbi_s": [], "score_call_s": [],
                                                        "gop_rel_gap": gap, "lpost_rel_gap": lgap})
for _ in range(REPEATS):
    for (P, T), (mels, ids, model, run, opt, coff, r) in cases.items():
        r["scores_s"].append(timed(lambda: al.score_packed(run))[1])
        r["torch_s"].append(timed(lambda: torch_scores(run))[1])
        r["viterbi_s"].append(timed(lambda: viterbi_launch(run, (P + 63) // 64 * 64, opt, coff))[1])
        r["score_call_s"].append(timed(lambda: al.score(mels, ids, (), model))[1])
for P, T in SIZES:
    r = cases[(P, T)][6]
    ts, tt, tv, tc = (statistics.median(r[k]) for k in ("scores_s", "torch_s", "viterbi_s", "score_call_s"))
    mb = V * B * T * 4 / 1e6
    r.update(scores_median_s=ts, torch_median_s=tt, viterbi_median_s=tv, score_call_median_s=tc, share_of_score_call=ts / tc,
             L_megabytes=mb, scores_above_viterbi=ts > tv)
    result["sizes"][f"{P}x{T}"] = r
    print(f"{P} x {T}, B = {B}, L {mb:.1f} MB: scores (2 launches, host-timed with a synchronise) {ts * 1e6:8.1f} us "
          f"[{min(r['scores_s']) * 1e6:.1f}, {max(r['scores_s']) * 1e6:.1f}] | torch ops {tt * 1e6:8.1f} us "
          f"[{min(r['torch_s']) * 1e6:.1f}, {max(r['torch_s']) * 1e6:.1f}] x{tt / ts:.1f} | Viterbi launch {tv * 1e6:8.1f} us | score() call "
          f"{tc * 1e3:.2f} ms, of which the scores {100 * ts / tc:.2f} %" + ("  <-- the scores cost MORE than the Viterbi launch" if ts > tv else ""))
print(json.dumps(result))
