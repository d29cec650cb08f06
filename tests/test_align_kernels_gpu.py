"""GPU suite: the forced-alignment kernels (csrc/kk_align.hip) behind PhoneAligner against the fp64 oracle
(kokoro_ruslan_amd.align_torch): degenerate shapes, code-word and wave edges, the workload's size, the kernel's limits, optional
tokens at the inner, first and last positions, the exact cases, the features, the log-likelihoods, the class statistics, bitwise batch
independence, the guards and the infeasible utterance.

As in test_dtw_gpu.py the kernel's path is not compared cell by cell with the oracle's: fp32 near-ties may legitimately choose
differently.  What pins the recurrence is the score.  Let S64 be the oracle's fp64 optimum ON THE KERNEL'S OWN fp32 L and A = sum_t
max_v |L(v, t)|.  The kernel's S(p, t) is a sequential fp32 sum of t + 1 terms along its path (max() selects, it does not round), so it
differs from that path's exact sum by at most (T - 1) u A (1 + O(T u)), u = 2^-24; the oracle's best path evaluated in fp32 loses as
little, so the two maxima differ by no more than that.  Doubled, as everywhere in this suite: |score - S64| <= T 2^-23 A, and the exact
fp64 score of the kernel's durations is >= S64 - T 2^-23 A (a path the kernel preferred cannot be worse than the optimum by more than
both roundings).

The log-likelihood L(v, t) = sum_d a (x - mu)^2 + c on the kernel's own fp32 parameters: the difference rounds once, its square twice
more (3 u relative on a term), the fmaf chain rounds once per step on partial sums bounded by sum_d |term|, the last addition once:
(D + 4) u (sum_d |term| + |c|), doubled to (D + 4) 2^-23 (...).  The features: a cepstrum is an M-term fmaf chain of products bounded by
|x|max (test_dtw_gpu's bound M u |x|max, table entries below 1), c_0 an M-term sum divided by M (the same bound); the mean over time
is formed in fp64 of such values and rounded once, the subtraction and the halved difference round once each on values bounded by
sqrt(2 M) |x|max: 2 M u |x|max + 4 u sqrt(2 M) |x|max, written (M + 2 sqrt(2 M)) 2^-23 |x|max."""
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
V, D, M = 59, 28, 80
OPT = 0                                                    # the optional class: no other token uses it
VARIANTS = ("none", "inner", "first", "last")


def _model(g, v, d, spread=1.0):
    return {"mean": (torch.randn(v, d, generator=g, dtype=torch.float64) * spread), "var": torch.rand(v, d, generator=g, dtype=torch.float64) * 1.5 + 0.5}


def _ids(g, P, variant):
    ids = torch.randint(1, V, (P,), generator=g)
    if variant == "inner":
        ids[1:P - 1:3] = OPT                               # (never two adjacent ones)
    elif variant == "first":
        ids[0] = OPT
    elif variant == "last":
        ids[P - 1] = OPT
    return ids


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import align as A
    limit = A.max_tokens()
    shapes = [(1, 1), (1, 7), (3, 3), (2, 1), (15, 40), (16, 40), (17, 40), (33, 70), (64, 64), (65, 200), (300, 1800),
              (limit, limit + 76), (5, 4096)]
    g = torch.Generator().manual_seed(23)
    al = A.PhoneAligner(n_classes=V)
    model = _model(g, V, D)
    items = [(P, T, var) for P, T in shapes for var in VARIANTS]
    feats = [torch.randn(T, D, generator=g) * 1.5 for P, T, _ in items]
    ids = [_ids(g, P, var) for P, _, var in items]
    run = al.run_packed(None, ids, (OPT,), model, feats=feats)           # one launch of each kernel for all items; read once, never changed
    torch.cuda.synchronize()
    host = {k: run[k].cpu().numpy() for k in ("L", "score", "end", "durations", "label")}
    cache = {}

    def item(n):
        """Everything about item n on the host: kernel outputs and the fp64 oracle on the kernel's fp32 L."""
        if n not in cache:
            f0, f1, p0, p1 = run["foff_host"][n], run["foff_host"][n + 1], run["poff_host"][n], run["poff_host"][n + 1]
            L = host["L"][:, f0:f1].astype(np.float64)
            i = ids[n].numpy()
            d64, S64 = R.align(L, i, i == OPT)
            cache[n] = dict(L=L, ids=i, opt=i == OPT, d64=d64, S64=S64, score=float(host["score"][n]), end=int(host["end"][n]),
                            dur=host["durations"][p0:p1].astype(np.int64), label=host["label"][f0:f1])
        return cache[n]
    return dict(limit=limit, items=items, al=al, model=model, item=item, A=A)


N_ITEMS = 13 * len(VARIANTS)


@pytest.mark.parametrize("n", range(N_ITEMS))
def test_durations_are_a_valid_path_that_scores_the_optimum(world, n):
    P, T, var = world["items"][n]
    r = world["item"](n)
    if r["d64"] is None:
        print(f"item {P} x {T} ({var}): infeasible")
        assert (P, T) == (2, 1) and var in ("none", "inner")
        assert r["score"] == -math.inf and r["end"] == -1 and not r["dur"].any() and (r["label"] == -1).all()
        return
    d = r["dur"]
    bound = T * EPS * float(np.abs(r["L"]).max(0).sum())
    got = R.path_score(r["L"], r["ids"], d) if int(d.sum()) == T and int(d.min()) >= 0 else -math.inf
    print(f"item {P} x {T} ({var}): score {r['score']!r}  S64 {r['S64']!r}  |difference| {abs(r['score'] - r['S64']):.3e}  "
          f"S64 - the fp64 score of the kernel's durations {r['S64'] - got:.3e}  bound {bound:.3e}  skipped {int((d == 0).sum())}")
    assert int(d.min()) >= 0 and int(d.sum()) == T
    assert not (d[~r["opt"]] == 0).any(), "only an optional token may get no frame"
    assert not ((d[1:] == 0) & (d[:-1] == 0)).any(), "two adjacent tokens are never both skipped"
    assert np.array_equal(r["label"], np.repeat(r["ids"], d)), "label must be the class of each frame's token"
    assert r["end"] == (P - 1 if d[P - 1] > 0 else P - 2)
    assert abs(r["score"] - r["S64"]) <= bound
    assert got >= r["S64"] - bound
    if P == T and var == "none":
        assert d.tolist() == [1] * P


def test_the_items_exercise_skips_at_every_position(world):
    """The shapes would prove little if no optional token were ever skipped (or kept) by the kernel."""
    seen = {v: [0, 0] for v in VARIANTS[1:]}
    for n, (P, T, var) in enumerate(world["items"]):
        r = world["item"](n)
        if var != "none" and r["d64"] is not None and P > 1:
            d, o = r["dur"], r["opt"]
            seen[var][0] += int((d[o] == 0).sum())
            seen[var][1] += int((d[o] > 0).sum())
    print(seen)
    for var, (skipped, kept) in seen.items():
        assert skipped > 0 and kept > 0, f"{var}: {skipped} skipped, {kept} kept"


def test_features_at_the_class_means_reproduce_the_generating_durations(world):
    g = torch.Generator().manual_seed(3)
    means = (torch.randn(V, D, generator=g) * 4.0).double()              # fp32 values: the distance to the right class is exactly 0
    model = {"mean": means, "var": torch.ones(V, D, dtype=torch.float64)}
    feats, ids, durs = [], [], []
    for P in (1, 9, 40, 130):
        i = torch.randperm(V - 1, generator=g)[torch.arange(P) % (V - 1)] + 1      # neighbours (and second neighbours) differ
        d = torch.randint(1, 9, (P,), generator=g)
        i[2:P - 2:4] = OPT
        d[2:P - 2:8] = 0                                                  # every second optional token has no frames
        if P > 4:
            i[0], d[0], i[P - 1], d[P - 1] = OPT, 0, OPT, 0               # ... and so have the first and the last token
        feats.append(means[torch.repeat_interleave(i, d)].float())
        ids.append(i), durs.append(d)
    i = torch.arange(33) % (V - 1) + 1                                    # P = T, no optional token
    feats.append(means[i].float()), ids.append(i), durs.append(torch.ones(33, dtype=torch.long))
    recs = world["al"].align(None, ids, (OPT,), model, feats=feats)
    c = float(-0.5 * D * math.log(2 * math.pi))
    for r, d, x in zip(recs, durs, feats):
        assert r["feasible"] and r["durations"].dtype == torch.int64 and r["durations"].tolist() == d.tolist()
        assert r["score"] == pytest.approx(c * x.shape[0], rel=x.shape[0] * EPS)
    assert sum(int((d == 0).sum()) for d in durs) >= 10


@pytest.mark.parametrize("d", [2, 28, 64])
@pytest.mark.parametrize("v", [2, 59, 256])
def test_feats_and_loglik_against_the_fp64_oracle(world, v, d):
    g = torch.Generator().manual_seed(1000 * v + d)
    K = d // 2 - 1
    al = world["A"].PhoneAligner(K=K, n_classes=v)
    mels = [torch.randn(T, M, generator=g) * 2.0 - 5.0 for T in (100, 31)]          # 131 frames: one partial workgroup, two utterances
    feat = al.features(mels)
    got = feat.cpu().numpy().astype(np.float64)
    assert got.shape == (d, 131)
    want = np.concatenate([R.features(m, K) for m in mels]).T
    xmax = float(torch.cat(mels).abs().max())
    err, tol = float(np.abs(got - want).max()), (M + 2 * math.sqrt(2 * M)) * EPS * xmax
    print(f"V {v} D {d}: features, max abs error {err:.3e}  tol {tol:.3e}")
    assert err <= tol
    model = _model(g, v, d, spread=float(np.abs(want).std()))
    L = al.loglik(feat, model).cpu().numpy().astype(np.float64)
    a, mu, c = (t.cpu().numpy().astype(np.float64) for t in al.params(model))       # the kernel's own fp32 parameters
    ref = R.loglik_from_params(got.T, a, mu, c)
    mag = np.stack([(np.abs(a[k]) * (got.T - mu[k]) ** 2).sum(1) + abs(c[k]) for k in range(v)])
    ratio = float((np.abs(L - ref) / ((d + 4) * EPS * mag)).max())
    print(f"V {v} D {d}: log-likelihoods, max error / tolerance {ratio:.3e}")
    assert L.shape == (v, 131) and ratio <= 1.0


def test_accumulate_counts_exactly_sums_in_fp64_and_repeats_bitwise(world):
    g = torch.Generator().manual_seed(9)
    T = 700
    feat = (torch.randn(D, T, generator=g) * 3.0 + 1.0).cuda().contiguous()
    lab = torch.randint(0, V, (T,), generator=g)
    lab[lab == 5] = 6                                                     # class 5 is absent
    lab[lab == 7] = 8
    lab[333] = 7                                                          # class 7 has a single frame
    lab[10:20] = -1                                                       # frames of an infeasible utterance count nowhere
    n, s1, s2 = world["al"].accumulate(feat, lab.to(torch.int32).cuda())
    n2, t1, t2 = world["al"].accumulate(feat, lab.to(torch.int32).cuda())
    for x, y in ((n, n2), (s1, t1), (s2, t2)):
        assert torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8)), "two runs must give the same bits"
    x = feat.cpu().numpy().astype(np.float64).T
    rn, r1, r2 = R.accumulate([x], [lab.numpy()], V)
    assert n.dtype == torch.int64 and n.cpu().tolist() == rn.tolist() and rn[5] == 0 and rn[7] == 1
    for got, ref, mag in ((s1, r1, np.abs(x)), (s2, r2, x ** 2)):
        got = got.cpu().numpy()
        for k in range(V):
            sel = lab.numpy() == k
            bound = max(int(sel.sum()), 1) * 2.0 ** -52 * mag[sel].sum(0)
            assert (np.abs(got[k] - ref[k]) <= bound).all(), k
    m = world["al"].estimate(n, s1, s2)
    ref = R.model_from_stats(rn, r1, r2)
    assert np.allclose(m["mean"].cpu().numpy(), ref["mean"], rtol=1e-12, atol=1e-12) and np.allclose(m["var"].cpu().numpy(), ref["var"], rtol=1e-10)


def _pieces(run, n):
    """Every output of utterance n of a run_packed() result, as host tensors."""
    f0, f1, p0, p1, c0, c1 = (run[k][n + j] for k in ("foff_host", "poff_host", "coff_host") for j in (0, 1))
    return [run["feat"][:, f0:f1].cpu().contiguous(), run["L"][:, f0:f1].cpu().contiguous(), run["score"][n:n + 1].cpu(), run["end"][n:n + 1].cpu(),
            run["codes"][c0:c1].cpu(), run["durations"][p0:p1].cpu(), run["label"][f0:f1].cpu()]


def test_an_utterances_outputs_do_not_depend_on_the_batch(world):
    al, limit = world["al"], world["limit"]
    shapes = [(1, 9), (33, 47), (limit - 7, limit + 90), (17, 16), (70, 300)]
    g = torch.Generator().manual_seed(5)
    mels = [torch.randn(T, M, generator=g) * 2.0 - 5.0 for _, T in shapes]
    ids = [_ids(g, P, "none" if P > T else "inner") for P, T in shapes]      # 17 mandatory tokens on 16 frames: infeasible
    model = _model(g, V, D, spread=3.0)
    batch = al.run_packed(mels, ids, (OPT,), model)
    rev = al.run_packed(mels[::-1], ids[::-1], (OPT,), model)
    names = ("feat", "L", "score", "end", "codes", "durations", "label")
    for n in range(len(shapes)):
        alone = _pieces(al.run_packed([mels[n]], [ids[n]], (OPT,), model), 0)
        feasible = shapes[n] != (17, 16)
        assert (int(alone[3]) >= 0) == feasible and (int(alone[5].sum()) == shapes[n][1]) == feasible
        for name, x, y, z in zip(names, alone, _pieces(batch, n), _pieces(rev, len(shapes) - 1 - n)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"utterance {n}: {name} differs in the batch"
            assert torch.equal(x.view(torch.uint8), z.view(torch.uint8)), f"utterance {n}: {name} differs in the reversed batch"


def test_the_infeasible_utterance_does_not_disturb_its_neighbours(world):
    al, model = world["al"], world["model"]
    g = torch.Generator().manual_seed(8)
    feats = [torch.randn(T, D, generator=g) for T in (30, 4, 12)]
    ids = [_ids(g, P, "none") for P in (7, 5, 12)]                        # 5 mandatory tokens on 4 frames
    recs = al.align(None, ids, (), model, feats=feats)
    assert recs[1] == {"durations": None, "score": -math.inf, "feasible": False}
    for n in (0, 2):
        alone = al.align(None, [ids[n]], (), model, feats=[feats[n]])[0]
        assert recs[n]["feasible"] and recs[n]["score"] == alone["score"] and torch.equal(recs[n]["durations"], alone["durations"])
        assert int(recs[n]["durations"].sum()) == feats[n].shape[0]
    assert recs[2]["durations"].tolist() == [1] * 12


def test_guards_raise_before_any_launch(world):
    from kokoro_ruslan_amd import lib as kk
    al, limit = world["al"], world["limit"]
    model = {"mean": torch.zeros(V, D, dtype=torch.float64), "var": torch.ones(V, D, dtype=torch.float64)}
    m, t = (lambda T, ch=M: torch.zeros(T, ch)), (lambda P: torch.ones(P, dtype=torch.long))
    before = kk.launches
    for mels, ids, match in (([torch.zeros(5)], [t(2)], "must be a float tensor"),
                             ([m(5), m(5, 129)], [t(2), t(2)], "utterance 1: 129 mel channels"),
                             ([m(4097)], [t(2)], "4097 frames"),
                             ([m(5), m(5)], [t(2), t(0)], "utterance 1: no tokens"),
                             ([m(5)], [t(limit + 1)], f"{limit + 1} tokens"),
                             ([m(5)], [torch.tensor([1, V])], "phoneme ids must lie in"),
                             ([m(5)], [torch.tensor([1, -1])], "phoneme ids must lie in"),
                             ([m(5), m(5)], [t(2)], "2 mel tensors for 1 token")):
        with pytest.raises(ValueError, match=match):
            al.align(mels, ids, (), model)
        with pytest.raises(ValueError, match=match):
            al.fit(mels, ids)
    with pytest.raises(ValueError, match="needs a model"):
        al.align([m(5)], [t(2)])
    with pytest.raises(ValueError, match="the model's mean"):
        al.align([m(5)], [t(2)], (), {"mean": torch.zeros(V, 8), "var": torch.ones(V, 8)})
    assert kk.launches == before
    assert limit == 1024
