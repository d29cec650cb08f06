"""CPU suite: the fp64 oracle of the DTW kernels (kokoro_ruslan_amd.dtw_torch) against a plain triple-loop DP and an independent DCT,
its exact cases, the host-side guards of MelAligner, evaluate()'s records and summary on a stub engine, and the kokoro-eval CLI's
argument errors and --split selection with the engine stubbed."""
import json
import math

import numpy as np
import pytest
import torch

from kokoro.cli import evaluate as cli
from kokoro.inference import evaluate as E
from kokoro.inference import synth as S
from kokoro_ruslan_amd import dtw_torch as R


def _loop_dtw(ca, cb):
    """The definition, cell by cell: D, and the path walked back with the tie-break diagonal, (i-1, j), (i, j-1)."""
    Ta, Tb = len(ca), len(cb)
    D = np.zeros((Ta, Tb))
    back = {}
    for i in range(Ta):
        for j in range(Tb):
            d = math.sqrt(sum((ca[i][k] - cb[j][k]) ** 2 for k in range(ca.shape[1])))
            if i == 0 and j == 0:
                D[i, j] = d
                continue
            best, arg = math.inf, None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pi >= 0 and pj >= 0 and D[pi, pj] < best:
                    best, arg = D[pi, pj], (pi, pj)
            D[i, j], back[(i, j)] = d + best, arg
    path = [(Ta - 1, Tb - 1)]
    while path[-1] != (0, 0):
        path.append(back[path[-1]])
    return D, path[::-1]


@pytest.mark.parametrize("Ta,Tb,seed", [(1, 1, 0), (1, 7, 1), (7, 1, 2), (2, 2, 3), (12, 9, 4), (9, 12, 5), (5, 5, 6), (11, 3, 7)])
def test_oracle_equals_the_triple_loop(Ta, Tb, seed):
    g = np.random.default_rng(seed)
    ca, cb = g.standard_normal((Ta, 4)), g.standard_normal((Tb, 4))
    if seed >= 5:                                           # a grid of few distinct values: ties that the tie-break has to settle
        ca, cb = np.round(ca), np.round(cb)
    D, path = _loop_dtw(ca, cb)
    total, p, D2 = R.dtw(ca, cb)
    np.testing.assert_allclose(D2, D, rtol=1e-14, atol=0)
    assert p.dtype == np.int32 and [tuple(x) for x in p.tolist()] == path
    assert total == D2[-1, -1]
    assert R.path_cost(ca, cb, p) == pytest.approx(total, rel=1e-13)


@pytest.mark.parametrize("M,K", [(80, 13), (20, 1), (20, 19), (80, 32)])
def test_mcep_oracle_is_the_orthonormal_dct2_without_c0(M, K):
    x = np.random.default_rng(M + K).standard_normal((17, M)) * 3 - 5
    got = R.mcep(torch.from_numpy(x), K)
    assert got.shape == (17, K) and got.dtype == np.float64
    try:
        from scipy.fftpack import dct
        want = dct(x, type=2, norm="ortho", axis=1)[:, 1:K + 1]
    except ImportError:
        want = np.array([[math.sqrt(2.0 / M) * sum(x[t, m] * math.cos(math.pi * k * (m + 0.5) / M) for m in range(M))
                          for k in range(1, K + 1)] for t in range(x.shape[0])])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        R.mcep(x, 33)


def test_self_alignment_is_free_and_diagonal():
    c = np.random.default_rng(0).standard_normal((37, 13))
    total, p, D = R.dtw(c, c)
    assert total == 0.0 and p.tolist() == [[i, i] for i in range(37)]


def test_frame_doubled_copy_is_free_and_twice_as_long():
    c = np.random.default_rng(1).standard_normal((23, 13))
    total, p, _ = R.dtw(c, np.repeat(c, 2, axis=0))
    assert total == 0.0 and len(p) == 46
    assert p.tolist() == [[j // 2, j] for j in range(46)]


def test_path_stats_are_the_sums_along_the_path():
    g = np.random.default_rng(2)
    xa, xb = g.standard_normal((6, 20)), g.standard_normal((9, 20))
    ca, cb = R.mcep(xa, 5), R.mcep(xb, 5)
    _, p, _ = R.dtw(ca, cb)
    mcd, l1 = R.path_stats(ca, cb, xa, xb, p)
    want_mcd = sum(10 / math.log(10) * math.sqrt(2) * math.sqrt(sum((ca[i] - cb[j]) ** 2)) for i, j in p)
    want_l1 = sum(np.abs(xa[i] - xb[j]).mean() for i, j in p)
    assert mcd == pytest.approx(want_mcd, rel=1e-13) and l1 == pytest.approx(want_l1, rel=1e-13)


def test_oracle_on_a_pair_of_a_few_hundred_frames():
    g = np.random.default_rng(3)
    ca, cb = g.standard_normal((450, 13)), g.standard_normal((400, 13))
    total, p, D = R.dtw(ca, cb)
    assert D.shape == (450, 400) and 450 <= len(p) <= 849 and p[0].tolist() == [0, 0] and p[-1].tolist() == [449, 399]
    assert set(map(tuple, np.diff(p, axis=0).tolist())) <= {(1, 1), (1, 0), (0, 1)}
    assert R.path_cost(ca, cb, p) == pytest.approx(total, rel=1e-12)
    assert total <= R.path_cost(ca, cb, [(min(s, 449), max(0, s - 449)) for s in range(849)])      # (no worse than down, then along)


# ---- MelAligner's guards run before anything touches the device -----------------------------------------------------------------

def test_aligner_guards_need_no_device():
    from kokoro_ruslan_amd.dtw import MelAligner, dir_words
    a = MelAligner(device="cpu")
    m = lambda t, c=8: torch.zeros(t, c)
    with pytest.raises(ValueError, match="pair 1: the synthesized mel is empty"):
        a.align([m(3), m(0)], [m(3), m(3)])
    with pytest.raises(ValueError, match="pair 0: the reference mel has 4097 frames"):
        a.align([m(3)], [m(4097)])
    with pytest.raises(ValueError, match="pair 0: 8 synthesized mel channels against 9"):
        a.align([m(3)], [m(3, 9)])
    with pytest.raises(ValueError, match="differ in mel channels"):
        a.align([m(3), m(3, 9)], [m(3), m(3, 9)])
    with pytest.raises(ValueError, match="2 synthesized mels for 1"):
        a.align([m(3), m(3)], [m(3)])
    with pytest.raises(ValueError, match="pair 1: 40 x 17 frames need 1280 direction cells"):
        a.align([m(3), m(40)], [m(3), m(17)], max_cells=1279)
    with pytest.raises(ValueError):
        MelAligner(device="cpu", K=33)
    assert dir_words(3, 16) == 3 and dir_words(3, 17) == 6 and dir_words(1, 1) == 1
    assert a.align([], []) == []


# ---- evaluate() on a stub engine ------------------------------------------------------------------------------------------------

class StubEngine:
    """Utterance u -> a mel of sum(u) frames filled with len(u); bound = (1, sum(u), self.cap)."""
    device = "cpu"

    class dims:
        mel = 4

    def __init__(self, cap=100):
        self.calls, self.cap = [], cap

    def _run(self, utterances):
        mels = [torch.full((min(int(u.sum()), self.cap), 4), float(u.numel())) for u in utterances]
        info = {"durations": [u.clone().float() for u in utterances], "T": [int(u.sum()) for u in utterances],
                "bounds": [(1, int(u.sum()), self.cap) for u in utterances]}
        return mels, info

    def generate_batch(self, utterances, stress=None, *, want_info=False, **kw):
        self.calls.append(("batch", len(utterances), kw))
        return self._run(utterances) if want_info else self._run(utterances)[0]

    def generate_stream(self, utterances, stress=None, *, slots=32, want_info=False, **kw):
        self.calls.append(("stream", len(utterances), slots, kw))
        return self._run(utterances) if want_info else self._run(utterances)[0]


class StubAligner:
    """mcd_dtw = |Ta - Tb|, mel_l1_dtw = 0.5 |Ta - Tb|: enough to see every record routed to its own pair."""

    def align(self, syn, ref, **kw):
        return [{"total": 0.0, "steps": max(len(s), len(r)), "mcd_dtw": float(abs(len(s) - len(r))),
                 "mel_l1_dtw": 0.5 * abs(len(s) - len(r)), "len_ratio": len(s) / len(r)} for s, r in zip(syn, ref)]


UTTS = [torch.tensor([3, 4, 5]), torch.tensor([7]), torch.tensor([1, 2]), torch.tensor([30, 30])]
REFS = [torch.zeros(10, 4), torch.zeros(7, 4), torch.zeros(6, 4), torch.zeros(40, 4)]
DURS = [torch.tensor([3, 4, 4]), torch.tensor([7]), torch.tensor([2, 4]), torch.tensor([20, 20])]


@pytest.mark.parametrize("stream", [True, False])
def test_evaluate_records_and_summary(stream):
    e = StubEngine(cap=50)
    recs, summ = E.evaluate(e, UTTS, None, REFS, stream=stream, slots=5, batch_size=3, durations=DURS, names=list("abcd"),
                            aligner=StubAligner(), max_len=77)
    if stream:
        assert e.calls == [("stream", 4, 5, {"max_len": 77})]
    else:
        assert [c[:2] for c in e.calls] == [("batch", 3), ("batch", 1)] and all(c[2] == {"max_len": 77} for c in e.calls)
    assert [r["name"] for r in recs] == list("abcd")
    assert [r["frames"] for r in recs] == [12, 7, 3, 50] and [r["ref_frames"] for r in recs] == [10, 7, 6, 40]
    assert [r["hit_bound"] for r in recs] == [False, False, False, True]
    assert [r["mcd_dtw"] for r in recs] == [2.0, 0.0, 3.0, 10.0] and [r["mel_l1_dtw"] for r in recs] == [1.0, 0.0, 1.5, 5.0]
    assert [r["len_ratio"] for r in recs] == [1.2, 1.0, 0.5, 1.25]
    assert [r["dur_abs_err"] for r in recs] == [1.0, 0.0, 3.0, 20.0]
    assert summ["utterances"] == 4 and summ["hit_bound_share"] == 0.25
    assert summ["mcd_dtw"]["mean"] == 3.75 and summ["mcd_dtw"]["median"] == 2.5
    assert summ["mcd_dtw"]["p95"] == pytest.approx(float(np.percentile([2.0, 0.0, 3.0, 10.0], 95)))
    assert summ["dur_abs_err"]["mean"] == 6.0 and summ["len_ratio"]["p95"] == pytest.approx(float(np.percentile([1.2, 1.0, 0.5, 1.25], 95)))


def test_evaluate_without_durations_and_its_argument_errors():
    e = StubEngine()
    recs, summ = E.evaluate(e, UTTS, None, REFS, aligner=StubAligner())
    assert [r["name"] for r in recs] == [0, 1, 2, 3] and "dur_abs_err" not in recs[0] and "dur_abs_err" not in summ
    assert not any(r["hit_bound"] for r in recs) and summ["hit_bound_share"] == 0.0
    assert E.evaluate(e, [], None, [], aligner=StubAligner()) == ([], {"utterances": 0, "hit_bound_share": 0.0})
    with pytest.raises(ValueError):
        E.evaluate(e, UTTS, None, REFS[:3], aligner=StubAligner())
    with pytest.raises(ValueError):
        E.evaluate(e, UTTS, None, REFS, durations=DURS[:2], aligner=StubAligner())
    with pytest.raises(ValueError):
        E.evaluate(e, UTTS, None, REFS, slots=0, aligner=StubAligner())
    with pytest.raises(ValueError):
        E.evaluate(e, UTTS, None, REFS, stream=False, batch_size=0, aligner=StubAligner())


# ---- the CLI --------------------------------------------------------------------------------------------------------------------

BASE = ["--checkpoint", "c", "--features", "d"]


@pytest.mark.parametrize("extra", [["--indices", "1", "--split", "val"], ["--indices"], ["--indices", "-1"], ["--validation-split", "0"],
                                   ["--validation-split", "1.0"], ["--slots", "4", "--no-stream"], ["--batch-size", "4"],
                                   ["--slots", "0"], ["--no-stream", "--batch-size", "0"], ["--mcep", "0"], ["--mcep", "33"],
                                   ["--split", "test"], ["--weights", "best"]])
def test_argument_errors_go_through_parser_error(extra, capsys):
    p = cli.build_parser()
    with pytest.raises(SystemExit) as ex:
        cli.check_args(p, p.parse_args(BASE + extra))
    assert ex.value.code == 2 and "error:" in capsys.readouterr().err


def test_parser_defaults():
    p = cli.build_parser()
    a = p.parse_args(BASE)
    cli.check_args(p, a)
    assert (a.split, a.validation_split, a.weights, a.math, a.no_stream, a.slots, a.batch_size, a.mcep, a.output) == \
        (None, 0.1, "auto", "bf16", False, None, None, 13, None)
    assert (a.stop_threshold, a.max_len, a.min_len_ratio, a.min_len_floor) == (None, None, None, None)


def _write_cache(d, n):
    from kokoro.data.cached import FEATURE_CACHE_VERSION
    for i in range(n):
        T, P = 5 + i, 2 + i % 3                              # distinct lengths: the length-sorted order is the file order
        dur = torch.ones(P, dtype=torch.int64)
        dur[-1] = T - (P - 1)
        torch.save({"mel_spec": torch.full((4, T), float(i)), "phoneme_indices": torch.arange(1, P + 1), "stress_indices": torch.zeros(P, dtype=torch.int64),
                    "phoneme_durations": dur, "stop_token_targets": torch.zeros(T), "pitch": torch.zeros(T), "energy": torch.zeros(T),
                    "mel_length": T, "phoneme_length": P, "text": "", "audio_file": f"u{i:02d}.wav", "_cache_version": FEATURE_CACHE_VERSION},
                   d / f"u{i:02d}.pt")


@pytest.mark.parametrize("extra,which", [([], "val"), (["--split", "val"], "val"), (["--split", "train"], "train"), (["--split", "all"], "all"),
                                         (["--indices", "4", "1"], "indices"), (["--split", "val", "--validation-split", "0.25"], "val25")])
def test_kokoro_eval_selects_the_trainers_split_and_writes_the_report(tmp_path, monkeypatch, extra, which):
    from kokoro.data.cached import split_indices
    cache = tmp_path / "cache"
    cache.mkdir()
    _write_cache(cache, 20)
    train, val = split_indices(20, 0.1)
    want = {"val": val, "train": train, "all": list(range(20)), "indices": [4, 1], "val25": split_indices(20, 0.25)[1]}[which]
    assert len(val) == 2 and not set(val) & set(train)
    e = StubEngine()
    monkeypatch.setattr(S, "load_for_inference", lambda path, **kw: (e, S.InferenceControls(max_len=40), "ema"))
    seen = {}
    real = E.evaluate

    def spy(engine, ids, stress, ref_mels, **kw):
        seen.update(kw, n=len(ids), ref=[float(m[0, 0]) for m in ref_mels], shapes=[tuple(m.shape) for m in ref_mels])
        return real(engine, ids, stress, ref_mels, aligner=StubAligner(), **kw)
    monkeypatch.setattr(E, "evaluate", spy)
    out = tmp_path / "report.json"
    assert cli.main(["--checkpoint", "ck", "--features", str(cache), "--output", str(out), "--slots", "6"] + extra) == 0
    assert seen["ref"] == [float(i) for i in want], "the ground-truth mels of exactly the selected utterances, in that order"
    assert seen["shapes"] == [(5 + i, 4) for i in want], "mels are handed over frame-major"
    assert seen["stream"] is True and seen["slots"] == 6 and seen["max_len"] == 40 and seen["mcep"] == 13
    assert [int(d.sum()) for d in seen["durations"]] == [5 + i for i in want]
    rep = json.loads(out.read_text())
    assert [r["name"] for r in rep["records"]] == [f"u{i:02d}" for i in want]
    assert rep["weights"] == "ema" and rep["controls"]["max_len"] == 40 and rep["summary"]["utterances"] == len(want)
    assert rep["split"] == ("indices" if which == "indices" else which.rstrip("25"))
    assert set(rep["summary"]) >= {"mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err", "hit_bound_share", "utterances"}


def test_kokoro_eval_no_stream_and_mel_mismatch(tmp_path, monkeypatch, capsys):
    cache = tmp_path / "cache"
    cache.mkdir()
    _write_cache(cache, 12)
    e = StubEngine()
    monkeypatch.setattr(S, "load_for_inference", lambda path, **kw: (e, S.InferenceControls(), "model"))
    real = E.evaluate
    monkeypatch.setattr(E, "evaluate", lambda *a, **kw: real(*a, aligner=StubAligner(), **kw))
    assert cli.main(BASE[:2] + ["--features", str(cache), "--no-stream", "--batch-size", "5", "--split", "all"]) == 0
    assert [c[:2] for c in e.calls] == [("batch", 5), ("batch", 5), ("batch", 2)]
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("kokoro-eval: 12 utterances (model weights")
    assert [ln.split()[0] for ln in lines[1:5]] == ["mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err"]
    e.dims = type("dims", (), {"mel": 80})
    with pytest.raises(SystemExit):
        cli.main(BASE[:2] + ["--features", str(cache), "--split", "all"])
