"""CPU suite: the fp64 oracle of the forced alignment (kokoro_ruslan_amd.align_torch) on synthetic corpora with a known alignment and
on hand-built score tables, and kokoro-align's host side (flag checks, reading a cache, replacing an entry's durations).

The corpora are align_torch.synthetic_corpus: 40 utterances, 12 classes, 8 dimensions, class means N(0, 2^2), noise 0.5, 5-20 tokens of
1-12 frames.  The two accuracy caps are the issue's: a numpy prototype of the specification labelled 100 % of the frames correctly
without optional tokens and 98.8-99.9 % with a quarter of the inner tokens optional, half of them zero-length."""
import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R


@pytest.fixture(scope="module")
def fits():
    out = {}
    for optional in (False, True):
        for seed in range(4):
            feats, ids, opts, durs, _ = R.synthetic_corpus(seed, optional)
            out[(optional, seed)] = (feats, ids, opts, durs) + R.fit(feats, ids, opts if optional else None, V=12)
    return out


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("optional,cap", [(False, 0.99), (True, 0.97)])
def test_fit_recovers_the_generating_alignment(fits, optional, cap, seed):
    feats, ids, opts, truth, model, durs, scores = fits[(optional, seed)]
    acc = R.frame_accuracy(ids, durs, truth)
    print(f"optional {optional} seed {seed}: frame accuracy {acc:.4f} after {len(scores)} passes, scores {[round(s, 1) for s in scores]}")
    assert acc >= cap
    assert all(b >= a for a, b in zip(scores, scores[1:])), "the corpus score must not decrease from one pass to the next"
    assert len(scores) < 6, "the labels are fixed within 3 passes: fit must have stopped early"
    for x, i, d in zip(feats, ids, durs):
        assert d.dtype == np.int64 and d.shape == i.shape and int(d.sum()) == x.shape[0] and int(d.min()) >= 0
    if optional:
        assert any((d == 0).any() for d in durs), "some optional tokens of this corpus have no frames"
        for o, d in zip(opts, durs):
            assert not (d[~o] == 0).any(), "only an optional token may get no frame"
    assert model["mean"].shape == model["var"].shape == (12, 8) and float(model["var"].min()) > 0.0


def test_fit_stops_once_the_durations_are_fixed(fits):
    feats, ids, opts, truth, model, durs, scores = fits[(False, 0)]
    _, again, more = R.fit(feats, ids, None, V=12, iters=50)
    assert len(more) == len(scores) < 6 and all(np.array_equal(a, b) for a, b in zip(durs, again))
    _, _, one = R.fit(feats, ids, None, V=12, iters=1)
    assert one == scores[:1]


def test_degenerate_shapes():
    g = np.random.default_rng(0)
    d, s = R.viterbi(g.normal(size=(7, 7)))
    assert d.tolist() == [1] * 7 and np.isfinite(s)
    L = g.normal(size=(1, 9))
    d, s = R.viterbi(L)
    assert d.tolist() == [9] and s == pytest.approx(L.sum())
    assert R.viterbi(g.normal(size=(1, 1)))[0].tolist() == [1]
    assert R.viterbi(g.normal(size=(4, 3))) == (None, -np.inf), "more mandatory tokens than frames"
    d, _ = R.viterbi(g.normal(size=(3, 2)), [False, True, False])
    assert d.tolist() == [1, 0, 1]
    assert R.viterbi(g.normal(size=(4, 2)), [False, True, True, False]) == (None, -np.inf), "two adjacent optional tokens are never both skipped"
    with pytest.raises(ValueError):
        R.viterbi(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        R.viterbi(np.zeros((2, 3)), [True])


def test_start_rule_on_hand_built_tables():
    """optional[0], P = T = 3.  Taking token 0 leaves one frame each; skipping it starts at token 1."""
    opt = [True, False, False]
    d, s = R.viterbi([[-5, -5, -5], [0, 0, 0], [0, 0, 0]], opt)           # starting at token 1 is strictly better: taken
    assert d.tolist() == [0, 1, 2] and s == 0.0
    d, s = R.viterbi([[0, 0, 0], [-5, 0, 0], [0, 0, 0]], opt)            # strictly worse (frame 0 dislikes token 1): not taken
    assert d.tolist() == [1, 1, 1] and s == 0.0
    d, s = R.viterbi([[9, 0, 0], [0, 0, 0], [0, 0, 0]], opt)             # token 0 claims frame 0
    assert d.tolist() == [1, 1, 1] and s == 9.0
    d, s = R.viterbi([[-5, -5, -5], [0, 0, 0], [0, 0, 0]], [False] * 3)   # without the flag there is no such start
    assert d.tolist() == [1, 1, 1] and s == -5.0


def test_end_rule_on_hand_built_tables():
    """optional[P-1], P = T = 3: the path may end at token 1, only when S(1, 2) is strictly greater than S(2, 2)."""
    opt = [False, False, True]
    d, s = R.viterbi([[0, 0, 0], [0, 0, 0], [-5, -5, -5]], opt)          # strictly greater: the last token is skipped
    assert d.tolist() == [1, 2, 0] and s == 0.0
    d, s = R.viterbi(np.zeros((3, 3)), opt)                               # equal: not taken
    assert d.tolist() == [1, 1, 1] and s == 0.0
    d, s = R.viterbi([[0, 0, 0], [0, 0, -1], [0, 0, 0]], opt)            # smaller: not taken
    assert d.tolist() == [1, 1, 1] and s == 0.0
    d, s = R.viterbi([[0, 0, 0], [0, 0, 0], [-5, -5, -5]], [False] * 3)
    assert d.tolist() == [1, 1, 1] and s == -5.0


def test_an_all_equal_table_resolves_to_stay_first():
    """Among equal candidates "stay" wins, so walking back from the end every token but the last keeps one frame."""
    assert R.viterbi(np.zeros((2, 4)))[0].tolist() == [1, 3]
    assert R.viterbi(np.zeros((3, 7)))[0].tolist() == [1, 1, 5]
    # the choice is made cell by cell: at (2, 1) the skip is the only finite candidate, and "stay" then keeps the path on it
    assert R.viterbi(np.zeros((3, 4)), [False, True, False])[0].tolist() == [1, 0, 3]
    # at (2, 2) "advance" and "skip" are equal and "stay" is worse: the later candidate must be strictly greater, so advance
    assert R.viterbi([[0, 0, 0], [0, 0, 0], [0, -9, 0]], [False, True, False])[0].tolist() == [1, 1, 1]


def test_features():
    z = R.features(np.full((8, 80), -5.0))                                # 8 equal frames: the sum and its mean are exact
    assert z.shape == (8, 28) and float(np.abs(z).max()) == 0.0
    assert float(np.abs(R.features(np.full((5, 20), 1.7), K=3)).max()) <= 1e-12
    g = np.random.default_rng(1)
    x = g.normal(size=(6, 20))
    f = R.features(x, K=4)
    assert f.shape == (6, 10) and np.allclose(f[:, :5].mean(0), 0.0, atol=1e-12)
    assert np.allclose(f[:, 4], x.mean(1) - x.mean())                     # column K is c_0, mean-normalised
    assert np.allclose(f[0, 5:], (f[1, :5] - f[0, :5]) / 2) and np.allclose(f[-1, 5:], (f[-1, :5] - f[-2, :5]) / 2)
    assert np.allclose(f[2, 5:], (f[3, :5] - f[1, :5]) / 2)
    assert np.allclose(R.features(x + 3.0, K=4)[:, :4], f[:, :4], atol=1e-9), "a constant offset only moves c_0, and its mean takes that"
    assert R.features(x[:1], K=4).shape == (1, 10) and float(np.abs(R.features(x[:1], K=4)).max()) == 0.0
    assert R.features(x, K=0).shape == (6, 2)


def test_estimation_rules():
    x = np.array([[0.0, 1.0], [2.0, 1.0], [4.0, 1.0], [10.0, 1.5]])
    n, s1, s2 = R.accumulate([x], [np.array([0, 0, 0, 2])], 4)
    assert n.tolist() == [3, 0, 1, 0] and s1[0].tolist() == [6.0, 3.0] and s2[0].tolist() == [20.0, 3.0]
    m = R.model_from_stats(n, s1, s2, var_floor=0.01)
    gmean, gvar = x.mean(0), x.var(0)
    assert np.allclose(m["mean"][0], [2.0, 1.0]) and np.allclose(m["var"][0], [8.0 / 3.0, 0.01 * gvar[1]])    # the second is floored
    for v in (1, 2, 3):                                                   # absent, and a single frame: the global statistics
        assert np.allclose(m["mean"][v], gmean) and np.allclose(m["var"][v], gvar)
    L = R.loglik(x, m)
    want = -0.5 * (((x - m["mean"][0]) ** 2 / m["var"][0]) + np.log(2 * np.pi * m["var"][0])).sum(1)
    assert L.shape == (4, 4) and np.allclose(L[0], want)
    assert R.path_score(L, [0, 2], [3, 1]) == pytest.approx(L[0, :3].sum() + L[2, 3])
    n2, _, _ = R.accumulate([x], [np.array([0, -1, -1, 2])], 4)
    assert n2.tolist() == [1, 0, 1, 0], "a label below 0 counts nowhere"


# ---- kokoro-align's host side --------------------------------------------------------------------------------------------------------

def test_kokoro_align_flag_checks(capsys):
    from kokoro.cli import align as cli
    p = cli.build_parser()
    a = p.parse_args(["--cache-dir", "x", "--optional-id", "3", "--optional-id", "7"])
    cli.check_args(p, a)
    assert a.optional_id == [3, 7] and a.iters == 6 and a.batch_size == 64 and a.var_floor == 0.01 and not a.write_cache
    assert p.parse_args(["--cache-dir", "x"]).optional_id == [], "--optional-id has no default"
    for bad in (["--iters", "0"], ["--batch-size", "0"], ["--var-floor", "1.5"], ["--optional-id", "59"], ["--mcep", "32"],
                ["--model-in", "a", "--model-out", "b"]):
        with pytest.raises(SystemExit):
            cli.check_args(p, p.parse_args(["--cache-dir", "x"] + bad))
    capsys.readouterr()


def test_kokoro_align_reads_a_cache_and_replaces_only_the_durations(tmp_path):
    from kokoro.cli import align as cli
    from kokoro.data import features as DF
    from kokoro.data.cached import reference_reconcile
    g = torch.Generator().manual_seed(0)
    for name, T, P in (("b", 9, 4), ("a", 5, 2)):
        ft = {"mel_spec": torch.randn(80, T, generator=g), "pitch": torch.rand(T, generator=g), "energy": torch.rand(T, generator=g),
              "mel_length": T}
        DF.write_cache_entry(str(tmp_path), DF.cache_entry(ft, name, torch.arange(P) + 1, None, None, "text " + name))
    entries = cli.read_cache(str(tmp_path))
    assert [e["name"] for e in entries] == ["a", "b"] and entries[1]["mel"].shape == (9, 80)
    assert entries[1]["durations"].tolist() == [3, 2, 2, 2]
    before = torch.load(entries[1]["path"], weights_only=False)
    new = torch.tensor([1, 0, 5, 3])
    cli.replace_durations(entries[1]["path"], new)
    after = torch.load(entries[1]["path"], weights_only=False)
    assert after["phoneme_durations"].tolist() == [1, 0, 5, 3] and after["phoneme_durations"].dtype == torch.long
    assert set(after) == set(before)
    for k, v in before.items():
        if k != "phoneme_durations":
            assert torch.equal(v, after[k]) if isinstance(v, torch.Tensor) else v == after[k], k
    assert sorted(f.name for f in tmp_path.glob("*.pt*")) == ["a.pt", "b.pt"], "no temporary file stays"
    # durations of a skipped token are 0 and reference_reconcile would lift them to 1: those of a path without skips pass unchanged
    d = torch.tensor([1, 2, 5, 1])
    assert torch.equal(reference_reconcile(d, 9), d)
