"""CPU suite: the pronunciation scores' fp64 oracle (kokoro_ruslan_amd.align_torch.scores) against a plain-loop restatement of the
definitions written here (nothing shared), on cases small enough to check by eye; what the scores mean, on the synthetic corpus: an
utterance scores higher on its own transcript than on a corrupted one; and the two tools' new flags."""
import math

import numpy as np
import pytest

from kokoro_ruslan_amd import align_torch as R


def _restated(L, ids, dur):
    """DESIGN §5 "Pronunciation scores", frame by frame and class by class."""
    L = np.asarray(L, dtype=np.float64)
    V, T = L.shape
    P = len(ids)
    tok = [dict(frames=0, gop_sum=0.0, lpost_sum=0.0, hits=0) for _ in range(P)]
    if dur is not None:
        owner = [p for p in range(P) for _ in range(int(dur[p]))]
        assert len(owner) == T
        for t in range(T):
            fmax, amax = L[0, t], 0
            for v in range(1, V):
                if L[v, t] > fmax:
                    fmax, amax = L[v, t], v
            z = 0.0
            for v in range(V):
                z += math.exp(L[v, t] - fmax)
            p = owner[t]
            margin = L[ids[p], t] - fmax
            tok[p]["frames"] += 1
            tok[p]["gop_sum"] += margin
            tok[p]["lpost_sum"] += margin - math.log(z)
            tok[p]["hits"] += int(amax == ids[p])
    tot = dict(gop=0.0, lpost=0.0, hits=0)
    for k in tok:
        tot["gop"] += k["gop_sum"]
        tot["lpost"] += k["lpost_sum"]
        tot["hits"] += k["hits"]
    return tok, tot


def _compare(L, ids, dur):
    got = R.scores(L, ids, dur)
    tok, tot = _restated(L, ids, dur)
    assert got["T"] == np.asarray(L).shape[1]
    assert got["frames"].tolist() == [k["frames"] for k in tok] and got["hits"].tolist() == [k["hits"] for k in tok]
    assert got["gop_sum"].tolist() == [k["gop_sum"] for k in tok], "margins are exact differences summed in frame order"
    for a, k in zip(got["lpost_sum"].tolist(), tok):
        # the oracle sums exp() over the classes with numpy's pairwise sum, the restatement one by one: V roundings of a sum <= V
        assert a == pytest.approx(k["lpost_sum"], rel=0, abs=max(k["frames"], 1) * L.shape[0] * 2.0 ** -52 * (1.0 + abs(k["lpost_sum"])))
    assert got["gop_total"] == tot["gop"] and got["hits_total"] == tot["hits"]
    assert got["lpost_total"] == pytest.approx(tot["lpost"], rel=1e-13, abs=1e-13)
    return got


def test_one_class_scores_exactly_zero():
    g = np.random.default_rng(0)
    L = g.normal(-30.0, 5.0, (1, 6)).astype(np.float32)
    got = _compare(L, [0, 0, 0], [1, 3, 2])
    assert got["gop_sum"].tolist() == [0.0] * 3 and got["lpost_sum"].tolist() == [0.0] * 3 and got["hits"].tolist() == [1, 3, 2]
    assert got["gop_total"] == 0.0 and got["lpost_total"] == 0.0 and got["hits_total"] == 6
    assert not got["margin"].any() and not got["lpost"].any() and not got["amax"].any()


def test_two_classes_by_hand():
    L = np.array([[-1.0, -5.0, -2.0], [-3.0, -4.0, -2.5]], dtype=np.float32)
    got = _compare(L, [0, 1], [2, 1])
    assert got["amax"].tolist() == [0, 1, 0]
    assert got["margin"].tolist() == [0.0, -1.0, -0.5]
    assert got["gop_sum"].tolist() == [-1.0, -0.5] and got["hits"].tolist() == [1, 0] and got["hits_total"] == 1
    want = [-math.log(1 + math.exp(-2.0)), -1.0 - math.log(1 + math.exp(-1.0)), -0.5 - math.log(1 + math.exp(-0.5))]
    assert got["lpost"].tolist() == pytest.approx(want, abs=1e-15)
    assert got["lpost_sum"].tolist() == pytest.approx([want[0] + want[1], want[2]], abs=1e-15)
    assert got["gop_total"] == -1.5


def test_a_tie_goes_to_the_lower_class_and_a_forced_higher_class_misses_with_margin_zero():
    L = np.array([[-7.0, -2.0], [-4.0, -9.0], [-4.0, -2.0]], dtype=np.float32)       # frame 0: classes 1 and 2 tie; frame 1: 0 and 2
    got = _compare(L, [2, 2], [1, 1])
    assert got["amax"].tolist() == [1, 0]
    assert got["margin"].tolist() == [0.0, 0.0] and got["hits"].tolist() == [0, 0] and got["gop_total"] == 0.0
    low = _compare(L, [1, 0], [1, 1])
    assert low["hits"].tolist() == [1, 1] and low["margin"].tolist() == [0.0, 0.0]
    assert low["lpost"].tolist() == got["lpost"].tolist(), "the posterior of either of two equal classes is the same"


@pytest.mark.parametrize("dur", [[0, 2, 3, 1], [2, 0, 3, 1], [2, 3, 1, 0], [0, 3, 0, 3], [0, 6, 0, 0]])
def test_tokens_without_frames_have_zeros_wherever_they_stand(dur):
    g = np.random.default_rng(4)
    L = g.normal(-20.0, 6.0, (5, 6)).astype(np.float32)
    ids = [3, 1, 4, 1]
    got = _compare(L, ids, dur)
    for p, d in enumerate(dur):
        if d == 0:
            assert (got["frames"][p], got["gop_sum"][p], got["lpost_sum"][p], got["hits"][p]) == (0, 0.0, 0.0, 0)
    assert got["frames"].tolist() == dur and (got["gop_sum"] <= 0).all() and (got["lpost_sum"] <= got["gop_sum"]).all()


def test_an_infeasible_utterance_has_zeros():
    L = np.random.default_rng(2).normal(0.0, 1.0, (4, 3)).astype(np.float32)
    got = _compare(L, [1, 2, 3, 0, 1], None)
    for k in ("frames", "gop_sum", "lpost_sum", "hits", "margin", "lpost"):
        assert not got[k].any(), k
    assert (got["gop_total"], got["lpost_total"], got["hits_total"], got["T"]) == (0.0, 0.0, 0, 3)
    for bad in ([1, 1, 1, 1, 0], [4, -1, 0, 0, 0], [1, 2]):                 # the wrong sum, a negative one, the wrong count
        with pytest.raises(ValueError, match="durations"):
            R.scores(L, [1, 2, 3, 0, 1], bad)


SEED, MEAN_STD, SHARE = 11, 2.0, 0.3


def test_the_true_transcript_scores_higher_than_a_corrupted_one_for_every_utterance():
    """synthetic_corpus(11, mean_std=2.0): 40 utterances of 12 classes.  The model is fitted by the oracle; every utterance is aligned
    and scored on its own tokens, and again on a copy in which 30 % of the tokens (at least one) are replaced by another class, the
    token count kept.  A replaced token's frames lie, in expectation, |mu_a - mu_b|^2 / (2 noise^2) = D mean_std^2 / noise^2 = 128
    below the best class; the alignment can hand some of them to the neighbours, never all."""
    feats, ids, _, durs, means = R.synthetic_corpus(SEED, mean_std=MEAN_STD)
    V = means.shape[0]
    model, fitted, _ = R.fit(feats, ids, V=V)
    assert R.frame_accuracy(ids, fitted, durs) > 0.95
    g = np.random.default_rng(SEED + 1)
    gaps = []
    for x, i in zip(feats, ids):
        L = R.loglik(x, model)
        own = R.scores(L, i, R.align(L, i)[0])
        j = i.copy()
        at = g.choice(len(i), max(1, int(round(SHARE * len(i)))), replace=False)
        j[at] = (i[at] + g.integers(1, V, len(at))) % V
        assert (j[at] != i[at]).all()
        other = R.scores(L, j, R.align(L, j)[0])
        gaps.append(own["gop_total"] / own["T"] - other["gop_total"] / other["T"])
        assert own["hits_total"] / own["T"] > other["hits_total"] / other["T"]
    print(f"gop(true) - gop(corrupted): min {min(gaps):.3f}  median {float(np.median(gaps)):.3f}")
    assert len(gaps) == 40 and min(gaps) > 0.0


# ---- the tools' flags --------------------------------------------------------------------------------------------------------------

def test_kokoro_align_scores_flags(capsys):
    from kokoro.cli import align as cli
    p = cli.build_parser()
    plain = p.parse_args(["--cache-dir", "x"])
    assert sorted(vars(plain)) == sorted(["cache_dir", "iters", "optional_id", "batch_size", "var_floor", "mcep", "n_classes", "model_in",
                                          "model_out", "output", "write_cache"]), "without the flags the namespace is what it was"
    a = p.parse_args(["--cache-dir", "x", "--scores"])
    cli.check_args(p, a)
    assert a.scores is True and not hasattr(a, "worst")
    a = p.parse_args(["--cache-dir", "x", "--scores", "--worst", "3", "--model-in", "m.pt"])
    cli.check_args(p, a)
    assert a.worst == 3 and a.model_in == "m.pt"
    for bad in (["--worst", "3"], ["--scores", "--worst", "-1"]):
        with pytest.raises(SystemExit):
            cli.check_args(p, p.parse_args(["--cache-dir", "x"] + bad))
    capsys.readouterr()
    assert cli.SCORE_FIELDS == ("gop", "logpost", "phone_acc", "gop_min", "gop_min_token")


def test_kokoro_eval_pronunciation_flags(capsys):
    from kokoro.cli import evaluate as cli
    base = ["--checkpoint", "c", "--features", "d"]
    p = cli.build_parser()
    plain = p.parse_args(base)
    cli.check_args(p, plain)
    for k in ("pronunciation", "align_iters", "optional_id", "pronunciation_tokens"):
        assert not hasattr(plain, k), f"without the flags the namespace is what it was: {k}"
    a = p.parse_args(base + ["--pronunciation"])
    cli.check_args(p, a)
    assert a.pronunciation == "" and not hasattr(a, "align_iters")
    a = p.parse_args(base + ["--pronunciation", "m.pt", "--optional-id", "3", "--optional-id", "7", "--pronunciation-tokens"])
    cli.check_args(p, a)
    assert a.pronunciation == "m.pt" and a.optional_id == [3, 7] and a.pronunciation_tokens is True
    a = p.parse_args(["--pronunciation"] + base + ["--align-iters", "2"])
    cli.check_args(p, a)
    assert a.pronunciation == "" and a.align_iters == 2
    a = p.parse_args(["--pronunciation=m.pt"] + base)
    assert a.pronunciation == "m.pt"
    for bad, message in ((["--align-iters", "2"], "--align-iters needs --pronunciation"),
                         (["--optional-id", "2"], "--optional-id needs --pronunciation"),
                         (["--pronunciation-tokens"], "--pronunciation-tokens needs --pronunciation"),
                         (["--pronunciation", "m.pt", "--align-iters", "2"], "--align-iters is for fitting a model"),
                         (["--pronunciation", "--align-iters", "0"], "--align-iters must be >= 1"),
                         (["--pronunciation", "--optional-id", "-1"], "--optional-id must be a phoneme id >= 0")):
        with pytest.raises(SystemExit) as ex:
            cli.check_args(p, p.parse_args(base + bad))
        assert ex.value.code == 2 and f"error: {message}" in capsys.readouterr().err


def test_token_lists_and_the_summary_of_pronunciation_records():
    import torch
    from kokoro.cli.evaluate import token_lists
    from kokoro.inference import evaluate as E
    rec = {"tokens": {"frames": torch.tensor([2, 0]), "hits": torch.tensor([1, 0]),
                      "gop": torch.tensor([-0.5, math.nan], dtype=torch.float64), "logpost": torch.tensor([-1.5, math.nan], dtype=torch.float64)}}
    assert token_lists(rec) == {"frames": [2, 0], "hits": [1, 0], "gop": [-0.5, None], "logpost": [-1.5, None]}
    assert token_lists({"tokens": None}) is None
    recs = [{"gop": -1.0, "ref_gop": -0.5, "gop_gap": -0.5, "phone_acc": 0.5, "phone_acc_gap": -0.25, "gop_min_token": 3},
            {"gop": None, "ref_gop": -0.25, "gop_gap": None, "phone_acc": None, "phone_acc_gap": None, "gop_min_token": None}]
    s = E.summarize(recs)
    assert s["pron_infeasible"] == 1 and s["gop"]["mean"] == -1.0 and s["ref_gop"]["mean"] == -0.375 and s["gop_gap"]["median"] == -0.5
    assert "gop_min_token" not in s and "pron_infeasible" not in E.summarize([{"mcd_dtw": 1.0}])
    assert set(E.PRON_METRICS) <= set(E.METRICS) and E.METRICS[:4] == ("mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err")
