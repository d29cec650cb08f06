"""GPU suite: kk_align_scores (csrc/kk_align.hip) behind PhoneAligner.score_packed / score against the fp64 oracle
(kokoro_ruslan_amd.align_torch.scores) evaluated on the kernel's OWN L, label and durations, read back: degenerate shapes, code-word
and wave edges, the workload's size, the kernels' limits, class counts around the 16-row chunks and the wave, tokens without frames at
the first, an inner and the last position, a constructed tie, bitwise batch independence, the infeasible utterance and the guards.
Every output is pre-filled with NaN / -1, so an element the kernels leave unwritten shows.

Exact: amax, hits, the margins, gop_sum per token and per utterance (compared as bits), and the zero rows.  A margin is ONE fp64
subtraction of two fp32 values and the sums run in the oracle's order from 0.0, so there is nothing to bound.

lpost_sum is bounded.  u = 2^-53.  The ROCm documentation of the device math library (HIP's math API reference,
docs/reference/math_api.rst, "Double precision mathematical functions"; ROCm installs no copy of it, so the figures are quoted) gives
exp and log a maximum error of 1 ULP each, a relative 2 u; the host's libm stays below 1 ULP as well.  Per frame, with S = sum_v
exp(L(v) - fmax) in [1, V]:
  * the arguments L(v) - max are fp64 differences of fp32 values, the same on both sides;
  * the kernel takes the classes 16 at a time and rescales its running sum by exp(old max - new max) when a chunk raises the maximum:
    R <= ceil(V / 16) - 1 times, each an exp (2 u) and a product (u); every term carries one exp (2 u); V additions round u S each:
    |dS| / S <= (2 + 3 R + V) u.  The oracle: 2 u and, for numpy's pairwise sum, no more than V u.  Together (4 + 3 R + 2 V) u;
  * log S lies in [0, ln 256 < 8), where an ULP is 2^-50 = 8 u: 8 u per side on top of dS / S;
  * lpost = margin - log S rounds once per side: 2 u |lpost|.
  e(t) = (2 V + 3 R + 20) u + 2 u |lpost(t)|.
A token's n frames are summed one by one on both sides: 2 (n - 1) u sum_t |lpost(t)| more.  An utterance's total adds its tokens'
bounds and 2 (P - 1) u sum_p |lpost_sum(p)|.  Doubled, as everywhere in this suite.  The tests assert that the bound stays below 1e-9
per frame: with V = 256 and |lpost| in the hundreds it is some 1e-13 + n 1e-13."""
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
V, D = 59, 28
OPT = 0
VARIANTS = ("none", "inner", "first", "last")
NAMES = ("margin", "lpost", "amax", "gop_sum", "lpost_sum", "hits", "utt_gop", "utt_lpost", "utt_hits")


def _bits(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).view(torch.int64)


def _frame_bound(v, lpost):
    return (2 * v + 3 * ((v + 15) // 16 - 1) + 20) * U + 2 * U * np.abs(lpost)


def _check_item(what, v, want, got):
    """want: R.scores of one utterance; got: the kernel's slices {name: numpy} of the same utterance."""
    assert np.array_equal(got["amax"], want["amax"]), f"{what}: amax"
    assert torch.equal(_bits(got["margin"]), _bits(want["margin"])), f"{what}: margin bits"
    assert np.array_equal(got["hits"], want["hits"]), f"{what}: hits"
    assert torch.equal(_bits(got["gop_sum"]), _bits(want["gop_sum"])), f"{what}: gop_sum bits"
    assert torch.equal(_bits(got["utt_gop"]), _bits(want["gop_total"])), f"{what}: the utterance's gop bits"
    assert int(got["utt_hits"]) == want["hits_total"], f"{what}: the utterance's hits"
    e, al, first, worst, total = _frame_bound(v, want["lpost"]), np.abs(want["lpost"]), 0, 0.0, 0.0
    assert (np.abs(got["lpost"] - want["lpost"]) <= 2 * e).all(), f"{what}: lpost per frame"
    for p, n in enumerate(want["frames"].tolist()):
        if n == 0:
            assert got["gop_sum"][p] == 0.0 and got["lpost_sum"][p] == 0.0 and got["hits"][p] == 0, f"{what}: token {p} has no frames"
            assert not np.signbit(got["gop_sum"][p]) and not np.signbit(got["lpost_sum"][p])
            continue
        b = e[first:first + n].sum() + 2 * (n - 1) * U * al[first:first + n].sum()
        assert 2 * b <= 1e-9 * n, f"{what}: the derived bound {2 * b:.3e} of token {p} exceeds 1e-9 per frame"
        err = abs(got["lpost_sum"][p] - want["lpost_sum"][p])
        worst = max(worst, err / (2 * b))
        assert err <= 2 * b, f"{what}: lpost_sum of token {p}: error {err:.3e}, bound {2 * b:.3e}"
        first, total = first + n, total + b
    P = len(want["frames"])
    total += 2 * (P - 1) * U * np.abs(want["lpost_sum"]).sum()
    err = abs(float(got["utt_lpost"]) - want["lpost_total"])
    print(f"{what}: lpost_sum error / bound {worst:.3f}; the total's error {err:.3e}, bound {2 * total:.3e}")
    assert err <= 2 * total, f"{what}: the utterance's lpost"


def _launch(L, label, durations, ids, frames, tokens):
    """kk_align_scores on hand-made inputs (host tensors), every output pre-filled; returns the outputs on the host as numpy."""
    from kokoro_ruslan_amd import lib as kk
    dev = "cuda"
    T, P, B = int(L.shape[1]), int(ids.shape[0]), len(frames)
    foff, poff = kk.packed_offsets(frames, torch.int32, dev), kk.packed_offsets(tokens, torch.int32, dev)
    out = {"margin": torch.full((T,), math.nan, dtype=torch.float64, device=dev), "lpost": torch.full((T,), math.nan, dtype=torch.float64, device=dev),
           "amax": torch.full((T,), -1, dtype=torch.int32, device=dev),
           "gop_sum": torch.full((P,), math.nan, dtype=torch.float64, device=dev), "lpost_sum": torch.full((P,), math.nan, dtype=torch.float64, device=dev),
           "hits": torch.full((P,), -1, dtype=torch.int32, device=dev),
           "utt_gop": torch.full((B,), math.nan, dtype=torch.float64, device=dev), "utt_lpost": torch.full((B,), math.nan, dtype=torch.float64, device=dev),
           "utt_hits": torch.full((B,), -1, dtype=torch.int32, device=dev)}
    Ld = L.to(dev, torch.float32).contiguous()
    kk.call("kk_align_scores", Ld, T, int(L.shape[0]), label.to(dev, torch.int32), durations.to(dev, torch.int32), ids.to(dev, torch.int32),
            foff, poff, B, *[out[k] for k in NAMES])
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _slices(host, foff, poff, n):
    f, p = slice(foff[n], foff[n + 1]), slice(poff[n], poff[n + 1])
    return {"margin": host["margin"][f], "lpost": host["lpost"][f], "amax": host["amax"][f], "gop_sum": host["gop_sum"][p],
            "lpost_sum": host["lpost_sum"][p], "hits": host["hits"][p], "utt_gop": host["utt_gop"][n], "utt_lpost": host["utt_lpost"][n],
            "utt_hits": host["utt_hits"][n]}


def _model(g, v, d, spread=1.0):
    return {"mean": (torch.randn(v, d, generator=g, dtype=torch.float64) * spread), "var": torch.rand(v, d, generator=g, dtype=torch.float64) * 1.5 + 0.5}


def _ids(g, P, variant):
    ids = torch.randint(1, V, (P,), generator=g)
    if variant == "inner":
        ids[1:P - 1:3] = OPT
    elif variant == "first":
        ids[0] = OPT
    elif variant == "last":
        ids[P - 1] = OPT
    return ids


SHAPES = [(1, 1), (1, 7), (3, 3), (16, 40), (17, 40), (65, 200), (1024, 1100), (5, 4096)]
ITEMS = [(P, T, var) for P, T in SHAPES for var in VARIANTS] + [(300, 1800, "inner")]


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import align as A
    from kokoro_ruslan_amd import lib as kk
    limit = A.max_tokens()
    assert limit == 1024 and SHAPES[6] == (limit, limit + 76)
    g = torch.Generator().manual_seed(29)
    al = A.PhoneAligner(n_classes=V)
    model = _model(g, V, D)
    feats = [torch.randn(T, D, generator=g) * 1.5 for _, T, _ in ITEMS]
    ids = [_ids(g, P, var) for P, _, var in ITEMS]
    run = al.run_packed(None, ids, (OPT,), model, feats=feats)            # one launch of each kernel for all items; read once
    T_total, P_total, B = run["L"].shape[1], run["ids"].shape[0], len(ITEMS)
    out = {k: torch.full((n,), fill, dtype=dt, device="cuda") for k, n, fill, dt in (
        ("margin", T_total, math.nan, torch.float64), ("lpost", T_total, math.nan, torch.float64), ("amax", T_total, -1, torch.int32),
        ("gop_sum", P_total, math.nan, torch.float64), ("lpost_sum", P_total, math.nan, torch.float64), ("hits", P_total, -1, torch.int32),
        ("utt_gop", B, math.nan, torch.float64), ("utt_lpost", B, math.nan, torch.float64), ("utt_hits", B, -1, torch.int32))}
    kk.call("kk_align_scores", run["L"], T_total, V, run["label"], run["durations"], run["ids"], run["foff"], run["poff"], B,
            *[out[k] for k in NAMES])
    again = al.score_packed(run)                                         # the public path, on outputs of its own
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in out.items()}
    for k in NAMES:
        assert torch.equal(again[k].cpu().view(torch.uint8), out[k].cpu().view(torch.uint8)), f"score_packed: {k} differs from the entry point"
    host.update({k: run[k].cpu().numpy() for k in ("L", "label", "durations", "score")})
    return dict(al=al, A=A, model=model, run=run, host=host, ids=ids, limit=limit)


@pytest.mark.parametrize("n", range(len(ITEMS)))
def test_scores_equal_the_oracle_on_the_kernels_own_alignment(world, n):
    P, T, var = ITEMS[n]
    run, host = world["run"], world["host"]
    f0, f1, p0, p1 = run["foff_host"][n], run["foff_host"][n + 1], run["poff_host"][n], run["poff_host"][n + 1]
    assert host["score"][n] > -math.inf, "every item of this list can be aligned"
    dur = host["durations"][p0:p1].astype(np.int64)
    i = world["ids"][n].numpy()
    assert np.array_equal(host["label"][f0:f1], np.repeat(i, dur))
    want = R.scores(host["L"][:, f0:f1], i, dur)
    _check_item(f"item {P} x {T} ({var})", V, want, _slices(host, run["foff_host"], run["poff_host"], n))


def test_nothing_is_left_unwritten(world):
    host = world["host"]
    for k in NAMES:
        x = host[k]
        assert not (np.isnan(x).any() if x.dtype == np.float64 else (x < 0).any()), k


@pytest.mark.parametrize("v", [1, 2, 59, 64, 65, 256])
def test_class_counts_and_tokens_without_frames_on_hand_made_inputs(v):
    """The entry point alone: L, label and durations made here, tokens without frames at the first, an inner and the last position."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(100 + v)
    durs = [torch.tensor([0, 3, 1, 0, 5, 2, 0]), torch.tensor([4]), torch.tensor([2, 0, 70, 1, 0, 0, 190, 3]), torch.tensor([0, 1]),
            torch.tensor([1] * 70)]
    ids = [torch.randint(0, v, (len(d),), generator=g) for d in durs]
    frames, tokens = [int(d.sum()) for d in durs], [len(d) for d in durs]
    L = torch.randn(v, sum(frames), generator=g) * 3.0 - 90.0            # (close together: many classes weigh in every frame's sum)
    L[:, 5] = L[0, 5]                                                     # one frame on which every class ties
    label = torch.cat([torch.repeat_interleave(i, d) for i, d in zip(ids, durs)])
    host = _launch(L, label, torch.cat(durs), torch.cat(ids), frames, tokens)
    foff, poff = np.cumsum([0] + frames), np.cumsum([0] + tokens)
    Lh = L.numpy()
    for n in range(len(durs)):
        want = R.scores(Lh[:, foff[n]:foff[n + 1]], ids[n].numpy(), durs[n].numpy())
        _check_item(f"V {v}, utterance {n}", v, want, _slices(host, foff, poff, n))
    assert host["amax"][5] == 0 and host["margin"][5] == 0.0
    if v == 1:
        assert not host["margin"].any() and not host["lpost"].any() and not host["gop_sum"].any() and not host["lpost_sum"].any()
        assert host["hits"].tolist() == torch.cat(durs).tolist()


def test_a_tie_goes_to_the_lower_class():
    """Two classes equal at a frame: the lower id is amax, and a forced higher id is a miss with margin 0."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = torch.full((20, 4), -50.0)
    L[3, 0] = L[17, 0] = -2.0                                             # frame 0: 3 and 17 tie (two chunks of 16 apart)
    L[4, 1] = L[5, 1] = -1.0                                              # frame 1: 4 and 5 tie (inside a chunk)
    L[19, 2] = -3.0                                                       # frame 2: no tie
    L[0, 3] = L[19, 3] = -4.0                                             # frame 3: the first and the last class tie
    ids, dur = torch.tensor([17, 5, 19, 0]), torch.tensor([1, 1, 1, 1])
    host = _launch(L, ids.clone(), dur, ids, [4], [4])
    assert host["amax"].tolist() == [3, 4, 19, 0]
    assert host["margin"].tolist() == [0.0] * 4 and host["hits"].tolist() == [0, 0, 1, 1] and host["utt_hits"].tolist() == [2]
    assert host["gop_sum"].tolist() == [0.0] * 4 and host["utt_gop"].tolist() == [0.0]
    _check_item("tie", 20, R.scores(L.numpy(), ids.numpy(), dur.numpy()), _slices(host, [0, 4], [0, 4], 0))
    assert host["lpost"][0] == pytest.approx(-math.log(2.0 + 18 * math.exp(-48.0)), abs=1e-15)


def _score_pieces(al, run, n):
    sc = al.score_packed(run)
    f, p = slice(run["foff_host"][n], run["foff_host"][n + 1]), slice(run["poff_host"][n], run["poff_host"][n + 1])
    return [sc["margin"][f].cpu(), sc["lpost"][f].cpu(), sc["amax"][f].cpu(), sc["gop_sum"][p].cpu(), sc["lpost_sum"][p].cpu(), sc["hits"][p].cpu(),
            sc["utt_gop"][n:n + 1].cpu(), sc["utt_lpost"][n:n + 1].cpu(), sc["utt_hits"][n:n + 1].cpu()]


def test_an_utterances_scores_do_not_depend_on_the_batch(world):
    al = world["al"]
    g = torch.Generator().manual_seed(6)
    shapes = [(9, 40), (33, 300), (70, 263), (1, 5), (130, 700)]
    feats = [torch.randn(T, D, generator=g) * 1.5 for _, T in shapes]
    ids = [_ids(g, P, "inner") for P, _ in shapes]
    model = world["model"]
    x, i = feats[1], ids[1]
    alone = _score_pieces(al, al.run_packed(None, [i], (OPT,), model, feats=[x]), 0)
    assert alone[3].numel() == 33 and float(alone[6]) < 0.0
    for at in (0, 2, 4):
        fs, ii = list(feats), list(ids)
        fs[at], ii[at] = x, i
        got = _score_pieces(al, al.run_packed(None, ii, (OPT,), model, feats=fs), at)
        for name, a, b in zip(NAMES, alone, got):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name} differs at position {at} of a batch of five"


def test_an_infeasible_utterance_gets_zeros_and_none_and_disturbs_nothing(world):
    al, model = world["al"], world["model"]
    g = torch.Generator().manual_seed(8)
    feats = [torch.randn(T, D, generator=g) for T in (30, 4, 12)]
    ids = [_ids(g, P, "none") for P in (7, 5, 12)]                        # 5 mandatory tokens on 4 frames
    run = al.run_packed(None, ids, (), model, feats=feats)
    pieces = _score_pieces(al, run, 1)
    assert float(run["score"][1]) == -math.inf
    for name, x in zip(NAMES[3:], pieces[3:]):
        assert not x.any() and not torch.isnan(x.double()).any(), f"{name} of the infeasible utterance"
    assert not pieces[0].any() and not pieces[1].any(), "frames without a class have margin and lpost 0"
    recs = al.score(None, ids, (), model, feats=feats)
    assert recs[1] == {"score": -math.inf, "feasible": False, "durations": None, "gop": None, "logpost": None, "phone_acc": None,
                       "gop_min": None, "gop_min_token": None, "tokens": None}
    for n in (0, 2):
        lone = al.run_packed(None, [ids[n]], (), model, feats=[feats[n]])
        for name, a, b in zip(NAMES, _score_pieces(al, lone, 0), _score_pieces(al, run, n)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"utterance {n}: {name}"
        alone = al.score(None, [ids[n]], (), model, feats=[feats[n]])[0]
        r = recs[n]
        assert r["feasible"] and set(r) == set(recs[1]) and torch.equal(r["durations"], alone["durations"])
        assert all(r[k] == alone[k] for k in ("score", "gop", "logpost", "phone_acc", "gop_min", "gop_min_token"))


def test_score_records_follow_the_device_sums(world):
    """score(): the means are taken in Python from the sums; tokens without frames are NaN in the tensors and ignored by gop_min."""
    al = world["al"]
    g = torch.Generator().manual_seed(3)
    means = (torch.randn(V, D, generator=g) * 4.0).double()
    model = {"mean": means, "var": torch.ones(V, D, dtype=torch.float64)}
    i = torch.randperm(V - 1, generator=g)[:12] + 1
    d = torch.randint(1, 9, (12,), generator=g)
    i[0], d[0], i[5], d[5], i[11], d[11] = OPT, 0, OPT, 0, OPT, 0         # skipped at the first, an inner and the last position
    x = means[torch.repeat_interleave(i, d)].float() + 0.3 * torch.randn(int(d.sum()), D, generator=g)
    run = al.run_packed(None, [i], (OPT,), model, feats=[x])
    sc = al.score_packed(run)
    rec = al.score(None, [i], (OPT,), model, feats=[x])[0]
    T = int(d.sum())
    assert rec["durations"].tolist() == d.tolist() and rec["tokens"]["frames"].tolist() == d.tolist()
    assert rec["gop"] == float(sc["utt_gop"][0]) / T and rec["logpost"] == float(sc["utt_lpost"][0]) / T
    # (the other classes lie hundreds below: their posteriors vanish beside 1.0, so logpost may be exactly 0)
    assert rec["phone_acc"] == int(sc["utt_hits"][0]) / T == 1.0 and rec["gop"] == 0.0 and rec["logpost"] <= 0.0
    gs, fr = sc["gop_sum"].cpu(), d.to(torch.float64)
    assert torch.isnan(rec["tokens"]["gop"][[0, 5, 11]]).all() and torch.isnan(rec["tokens"]["logpost"][[0, 5, 11]]).all()
    keep = d > 0
    assert torch.equal(rec["tokens"]["gop"][keep], (gs / fr)[keep]) and rec["tokens"]["hits"].tolist() == d.tolist()
    assert rec["gop_min"] == 0.0 and rec["gop_min_token"] == 1, "the first of equal minima, tokens without frames ignored"


def test_guards_raise_before_any_launch(world):
    from kokoro_ruslan_amd import lib as kk
    al, limit, run = world["al"], world["limit"], world["run"]
    model = {"mean": torch.zeros(V, D, dtype=torch.float64), "var": torch.ones(V, D, dtype=torch.float64)}
    f, t = (lambda T: torch.zeros(T, D)), (lambda P: torch.ones(P, dtype=torch.long))
    before = kk.launches
    for feats, ids, match in (([f(5)], [t(limit + 1)], f"{limit + 1} tokens"), ([f(4097)], [t(2)], "4097 frames"),
                              ([f(5), f(5)], [t(2)], "2 features tensors for 1 token"), ([f(5)], [torch.tensor([1, V])], "phoneme ids must lie in")):
        with pytest.raises(ValueError, match=match):
            al.score(None, ids, (), model, feats=feats)
    with pytest.raises(ValueError, match="needs a model"):
        al.score(None, [t(2)], feats=[f(5)])
    with pytest.raises(ValueError, match="n_classes must be an integer in 1..256"):
        world["A"].PhoneAligner(n_classes=257)
    T_total = run["L"].shape[1]
    for change, match in (({"L": torch.zeros(257, T_total, device="cuda")}, "L must be fp32"),
                          ({"label": run["label"][:-1]}, "label must be int32"),
                          ({"durations": run["durations"][1:]}, "durations must be int32"),
                          ({"ids": run["ids"][:-1]}, "the offsets end at"),
                          ({"foff_host": run["foff_host"][:-1] + [T_total + 1]}, "the offsets end at"),
                          ({"foff_host": [0, T_total], "poff_host": [0, int(run["ids"].shape[0])], "foff": run["foff"][:2], "poff": run["poff"][:2]},
                           "tokens; at most")):
        with pytest.raises(ValueError, match=match):
            al.score_packed(dict(run, **change))
    assert kk.launches == before
