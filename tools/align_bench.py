#!/usr/bin/env python3
"""Throughput of the forced-alignment kernels.

PhoneAligner.align (features, log-likelihoods, Viterbi, backtrack and the read of the durations: everything an alignment costs) on 64
utterances of 100 tokens x 600 frames and of 300 x 1800, and one PhoneAligner.fit pass (accumulate, estimate, align) over 256 utterances
of 100 x 600, against two baselines: the same recurrence written with torch ops on the same GPU (all utterances of the batch per op,
one frame at a time, the recurrence alone: L given, no codes, no path), and the fp64 oracle (kokoro_ruslan_amd.align_torch) on the host
in 16 threads.  Beside every align call the kk_align_loglik (M = 1) and kk_align_accumulate launches alone (device events) on that
batch's features and labels.  Five repeats with the device paths interleaved inside every repeat; medians, with the spread.  The host
oracle runs once per size on 16 utterances.  One JSON line at the end.

    python tools/align_bench.py [repeats=5]
    python tools/align_bench.py [repeats=5] --states S
    python tools/align_bench.py [repeats=5] --mixtures M

With --states S (1, 2 or 3) the same two sizes are aligned with S states per phoneme instead: PhoneAligner(states=S).align as above, and
the Viterbi and the backtrack launch alone (device events) -- kk_align_viterbi with S states on L [V S, T] beside the same entry point
with 1 state on the same box and the same frames (on the maximum over each phoneme's states), interleaved inside every repeat; medians,
with the spread.

With --mixtures M (2 or 4) the three mixture launches alone (device events) on 64 x 600 and 64 x 1800 frames of 28 dimensions, for 59
classes (1 state) and 177 classes (3 states) of M Gaussians: kk_align_loglik at M beside kk_align_loglik at M = 1 on the G = C M rows
followed by torch.logsumexp over each class's M rows, kk_align_mix_labels, and kk_align_accumulate_mix beside kk_align_accumulate on G
classes; the two comparisons only where G <= 256, which kk_align_accumulate takes.  Interleaved inside every repeat; medians."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import align_torch as R
from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.align import PhoneAligner

_ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
_ap.add_argument("repeats", nargs="?", type=int, default=5)
_ap.add_argument("--states", type=int, choices=(1, 2, 3), default=None, metavar="S", help="states per phoneme: 1, 2 or 3")
_ap.add_argument("--mixtures", type=int, choices=(2, 4), default=None, metavar="M", help="Gaussians per class: 2 or 4")
_args = _ap.parse_args()
REPEATS, STATES, MIXTURES = _args.repeats, _args.states, _args.mixtures
SIZES, B, FIT_B, M, V = ((100, 600), (300, 1800)), 64, 256, 80, 59
al = PhoneAligner(n_classes=V)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def corpus(n, P, T, seed):
    """n utterances whose frames follow their tokens' class templates in an uneven split: an alignment worth finding."""
    g = torch.Generator().manual_seed(seed)
    templates = torch.randn(V, M, generator=g) * 2.0 - 5.0
    mels, ids = [], []
    for _ in range(n):
        i = torch.randint(0, V, (P,), generator=g)
        d = torch.ones(P, dtype=torch.long) + torch.bincount(torch.randint(0, P, (T - P,), generator=g), minlength=P)
        mels.append((templates[torch.repeat_interleave(i, d)] + 0.5 * torch.randn(T, M, generator=g)).cuda())
        ids.append(i)
    return mels, ids


def torch_viterbi(L, ids):
    """The scores [B] of the best paths with torch ops: L [V, B, T], ids [B, P]; no optional tokens."""
    Bn, P = ids.shape
    Lp = L.permute(1, 0, 2).gather(1, ids[:, :, None].expand(Bn, P, L.shape[2]))      # [B, P, T]
    S = torch.full((Bn, P + 1), float("-inf"), device=L.device)
    S[:, 1] = Lp[:, 0, 0]
    for t in range(1, L.shape[2]):
        S = torch.cat([S[:, :1], Lp[:, :, t] + torch.maximum(S[:, 1:], S[:, :-1])], 1)
    return S[:, P]


def device_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def states_bench(S):
    """--states S: the whole alignment with S states, and the S-state Viterbi and backtrack launches beside the 1-state Viterbi."""
    from kokoro_ruslan_amd.align import code_words
    als = PhoneAligner(n_classes=V, states=S)
    out, todo = {"repeats": REPEATS, "states": S, "align": {}}, []
    for P, T in SIZES:
        mels, ids = corpus(B, P, T, 1000 + P)
        model, _, _ = als.fit(mels, ids, iters=2)                   # warm-up, and a model worth aligning with
        run = als.run_packed(mels, ids, (), model)
        Ls, L1 = run["L"], run["L"].view(V, S, -1).amax(1).contiguous()
        opt = torch.zeros(B * P, dtype=torch.uint8, device="cuda")
        score, end = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        coff = {n: kk.packed_offsets([code_words(P, T, n)] * B).cuda() for n in {1, S}}
        codes = torch.empty(B * code_words(P, T, S), dtype=torch.int32, device="cuda")
        threads = (P + 63) // 64 * 64
        sdur = torch.empty(B * P, S, dtype=torch.int32, device="cuda") if S > 1 else None
        dur, label = torch.empty(B * P, dtype=torch.int32, device="cuda"), torch.empty(B * T, dtype=torch.int32, device="cuda")
        def many(Ls=Ls, run=run, opt=opt, coff=coff[S], threads=threads, score=score, end=end, codes=codes):
            kk.call("kk_align_viterbi", Ls, Ls.shape[1], run["ids"], opt, run["foff"], run["poff"], coff, B, threads, S, score, end, codes)

        def back(run=run, coff=coff[S], end=end, codes=codes, sdur=sdur, dur=dur, label=label):      # (after many: its codes and end)
            kk.call("kk_align_backtrack", codes, coff, run["foff"], run["poff"], run["ids"], end, B, S, sdur, dur, label)

        def one(L1=L1, run=run, opt=opt, coff=coff[1], threads=threads, score=score, end=end, codes=codes):
            kk.call("kk_align_viterbi", L1, L1.shape[1], run["ids"], opt, run["foff"], run["poff"], coff, B, threads, 1, score, end, codes)
        many(), back(), one()
        todo.append(((P, T), mels, ids, model, many, back, one,
                     {"align_s": [], "viterbi_states_ms": [], "backtrack_ms": [], "viterbi_1state_ms": []}))
    for _ in range(REPEATS):
        for _, mels, ids, model, many, back, one, r in todo:
            r["align_s"].append(timed(lambda: als.align(mels, ids, (), model))[1])   # (called at once: this pass's mels)
            r["viterbi_states_ms"].append(device_ms(many))
            r["backtrack_ms"].append(device_ms(back))
            r["viterbi_1state_ms"].append(device_ms(one))
    for (P, T), _, _, _, _, _, _, r in todo:
        ta, tm, tb, t1 = (statistics.median(r[k]) for k in ("align_s", "viterbi_states_ms", "backtrack_ms", "viterbi_1state_ms"))
        r.update(align_median_s=ta, utterances_per_s=B / ta, viterbi_states_median_ms=tm, backtrack_median_ms=tb, viterbi_1state_median_ms=t1,
                 ratio=tm / t1)
        out["align"][f"{P}x{T}"] = r
        print(f"{P} x {T}, B = {B}, {S} state(s): align {ta * 1e3:8.2f} ms [{min(r['align_s']) * 1e3:.2f}, {max(r['align_s']) * 1e3:.2f}] = "
              f"{B / ta:8.0f} utterances/s | Viterbi launch {tm:.3f} ms [{min(r['viterbi_states_ms']):.3f}, {max(r['viterbi_states_ms']):.3f}] "
              f"| backtrack launch {tb:.3f} ms [{min(r['backtrack_ms']):.3f}, {max(r['backtrack_ms']):.3f}] "
              f"| 1-state kernel {t1:.3f} ms [{min(r['viterbi_1state_ms']):.3f}, {max(r['viterbi_1state_ms']):.3f}] | x{tm / t1:.2f}")
    print(json.dumps(out))


def mixtures_bench(M):
    """--mixtures M: the likelihood, labels and accumulate launches of a mixture model, beside the single-Gaussian entry points."""
    D, out, todo = 28, {"repeats": REPEATS, "mixtures": M, "launches": {}}, []
    g = torch.Generator().manual_seed(11)
    for S in (1, 3):
        for _, T in SIZES:
            C, Tt = V * S, B * T
            G = C * M
            alm = PhoneAligner(n_classes=V, states=S, mixtures=M)
            w = torch.rand(C, M, generator=g, dtype=torch.float64) + 0.1
            model = {"mean": torch.randn(G, D, generator=g, dtype=torch.float64) * 2.0, "var": torch.rand(G, D, generator=g, dtype=torch.float64) + 0.5,
                     "weight": w / w.sum(1, keepdim=True), "mixtures": M, **({"states": S} if S > 1 else {})}
            a, mu, k = alm.params(model)
            feat = (torch.randn(D, Tt, generator=g) * 2.0).cuda().contiguous()
            label = torch.repeat_interleave(torch.randint(0, C, (Tt // 6,), generator=g), 6).to(torch.int32).cuda()     # runs of 6 frames
            L, rows = torch.empty(C, Tt, device="cuda"), torch.empty(G, Tt, device="cuda") if G <= 256 else None
            mixlabel = alm.mix_labels(feat, model, label)
            count, sums = torch.empty(G, dtype=torch.int64, device="cuda"), torch.empty(2, G, D, dtype=torch.float64, device="cuda")
            ws = torch.empty(kk.load().kk_align_accumulate_mix_ws_bytes(Tt, G), dtype=torch.uint8, device="cuda")
            fns = {"loglik_mix_ms": lambda feat=feat, Tt=Tt, C=C, a=a, mu=mu, k=k, L=L: kk.call("kk_align_loglik", feat, Tt, D, C, M, a, mu, k, L),
                   "mix_labels_ms": lambda feat=feat, Tt=Tt, C=C, a=a, mu=mu, k=k, label=label, mixlabel=mixlabel:
                       kk.call("kk_align_mix_labels", feat, Tt, D, C, M, a, mu, k, label, mixlabel),
                   "accumulate_mix_ms": lambda feat=feat, mixlabel=mixlabel, Tt=Tt, G=G, count=count, sums=sums, ws=ws:
                       kk.call("kk_align_accumulate_mix", feat, mixlabel, Tt, D, G, count, sums[0], sums[1], ws, ws.numel())}
            if G <= 256:
                def rows_then_logsumexp(feat=feat, Tt=Tt, G=G, C=C, a=a, mu=mu, k=k, rows=rows):
                    kk.call("kk_align_loglik", feat, Tt, D, G, 1, a, mu, k, rows)
                    return torch.logsumexp(rows.view(C, M, Tt), 1)
                fns["loglik_rows_logsumexp_ms"] = rows_then_logsumexp
                fns["accumulate_ms"] = lambda feat=feat, mixlabel=mixlabel, Tt=Tt, G=G, count=count, sums=sums: \
                    kk.call("kk_align_accumulate", feat, mixlabel, Tt, D, G, count, sums[0], sums[1])
            for fn in fns.values():
                fn()                                                    # warm-up
            todo.append((f"C{C}xM{M}_T{Tt}", fns, {name: [] for name in fns}))
    for _ in range(REPEATS):
        for _, fns, r in todo:
            for name, fn in fns.items():
                r[name].append(device_ms(fn))
    for key, fns, r in todo:
        med = {name.replace("_ms", "_median_ms"): statistics.median(v) for name, v in r.items()}
        out["launches"][key] = dict(r, **med)
        print(f"{key}: " + " | ".join(f"{name[:-3]} {statistics.median(v):.3f} ms [{min(v):.3f}, {max(v):.3f}]" for name, v in r.items()))
    print(json.dumps(out))


if STATES is not None:
    states_bench(STATES)
    sys.exit(0)
if MIXTURES is not None:
    mixtures_bench(MIXTURES)
    sys.exit(0)
result = {"repeats": REPEATS, "align": {}, "fit": {}}
cases = {}


def launches(run, model):
    """The likelihood and the statistics launch of a batch, each alone: (loglik, accumulate)."""
    feat, label, (D, Tt) = run["feat"], run["label"], run["feat"].shape
    a, mu, c = al.params(model)
    L, count = torch.empty(V, Tt, device="cuda"), torch.empty(V, dtype=torch.int64, device="cuda")
    sums = torch.empty(2, V, D, dtype=torch.float64, device="cuda")
    return (lambda: kk.call("kk_align_loglik", feat, Tt, D, V, 1, a, mu, c, L),
            lambda: kk.call("kk_align_accumulate", feat, label, Tt, D, V, count, sums[0], sums[1]))


for P, T in SIZES:
    mels, ids = corpus(B, P, T, 1000 + P)
    model, _, _ = al.fit(mels, ids, iters=2)                    # warm-up, and a model worth aligning with
    run = al.run_packed(mels, ids, (), model)
    L = run["L"].reshape(V, B, T).contiguous()
    idt = torch.stack(ids).cuda()
    ours, base = run["score"].cpu(), torch_viterbi(L, idt).cpu()
    gap = float(((ours - base).abs() / base.abs()).max())      # both sum T fp32 terms along a best path
    print(f"{P} x {T}: kernels against torch ops, largest relative difference of the scores {gap:.2e}"
          + ("" if gap <= T * 2.0 ** -22 else "  <-- MORE than two fp32 sums of T terms explain"))
    cases[(P, T)] = (mels, ids, model, L, idt, launches(run, model), {"kernel_s": [], "torch_s": [], "loglik_ms": [], "accumulate_ms": [],
                                                                      "scores_rel_gap": gap})
fit_mels, fit_ids = corpus(FIT_B, *SIZES[0], 7)
al.fit(fit_mels, fit_ids, iters=1)
fit_s = []
for _ in range(REPEATS):
    for key, (mels, ids, model, L, idt, (ll, acc), r) in cases.items():
        r["kernel_s"].append(timed(lambda: al.align(mels, ids, (), model))[1])
        r["torch_s"].append(timed(lambda: torch_viterbi(L, idt))[1])
        r["loglik_ms"].append(device_ms(ll))
        r["accumulate_ms"].append(device_ms(acc))
    fit_s.append(timed(lambda: al.fit(fit_mels, fit_ids, iters=1))[1])
torch.set_num_threads(1)                                        # 16 utterances side by side, one thread each
for P, T in SIZES:
    mels, ids, model, L, idt, _, r = cases[(P, T)]
    Lh, ih = L[:, :16].double().cpu().numpy(), [i.numpy() for i in ids[:16]]
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda n: R.align(Lh[:, n], ih[n])[1], range(16)))
        host = time.perf_counter() - t0
    tk, tt = statistics.median(r["kernel_s"]), statistics.median(r["torch_s"])
    tl, tc = statistics.median(r["loglik_ms"]), statistics.median(r["accumulate_ms"])
    r.update(kernel_median_s=tk, torch_median_s=tt, loglik_median_ms=tl, accumulate_median_ms=tc, utterances_per_s=B / tk, cells_per_s=B * P * T / tk, host_oracle_16_threads_utterances_per_s=16 / host)
    result["align"][f"{P}x{T}"] = r
    print(f"{P} x {T}, B = {B}: align {tk * 1e3:8.2f} ms [{min(r['kernel_s']) * 1e3:.2f}, {max(r['kernel_s']) * 1e3:.2f}] = {B / tk:8.0f} utterances/s = "
          f"{B * P * T / tk / 1e9:6.2f} G cells/s | torch ops (recurrence only) {tt * 1e3:8.1f} ms [{min(r['torch_s']) * 1e3:.1f}, {max(r['torch_s']) * 1e3:.1f}] | x{tt / tk:.1f} "
          f"| loglik launch {tl:.3f} ms [{min(r['loglik_ms']):.3f}, {max(r['loglik_ms']):.3f}] "
          f"| accumulate launch {tc:.3f} ms [{min(r['accumulate_ms']):.3f}, {max(r['accumulate_ms']):.3f}] "
          f"| fp64 oracle on the host (recurrence and path, L given), 16 utterances in 16 threads: {host:.2f} s = {16 / host:.1f} utterances/s")
tf = statistics.median(fit_s)
P, T = SIZES[0]
result["fit"] = {"utterances": FIT_B, "tokens": P, "frames": T, "pass_s": fit_s, "pass_median_s": tf, "frames_per_s": FIT_B * T / tf}
print(f"fit, one pass over {FIT_B} utterances of {P} x {T} (features, accumulate, estimate, align): {tf * 1e3:.1f} ms "
      f"[{min(fit_s) * 1e3:.1f}, {max(fit_s) * 1e3:.1f}] = {FIT_B * T / tf / 1e6:.2f} M frames/s")
print(json.dumps(result))
