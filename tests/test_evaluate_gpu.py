"""GPU suite: kokoro.inference.evaluate.evaluate on a tiny random-weight engine: synthesis through generate_stream / generate_batch,
alignment on the device, and the records' definitions on cases whose answer is known."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import kokoro_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = "duration_adaptor.variance_adaptor"
PHONEMES = (2, 9, 5, 23)
DUR_BIAS = 1.5                         # durations ~ e^1.5 per phoneme: rows of ten to a hundred frames
STOP_AT_MIN = dict(max_len=160, stop_threshold=0.0)       # the stop rule fires on the first frame it may: at the row's minimum length


def _fixture():                        # (the tiny model of the synthesis tests)
    fx = np.load(os.path.join(GOLDEN, "inference_tiny.npz"))
    d = O.ModelDims(*[int(x) for x in fx["dims"]])
    seed = int(fx["seed"])
    P = O.init_params(d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in P.items():
        if p.dim() == 1:
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    P[f"{VA}.duration_predictor.linear.bias"].fill_(DUR_BIAS)
    return d, P


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d, P = _fixture()
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g).cuda() for n in PHONEMES]
    st = [torch.randint(0, 3, (n,), generator=g).cuda() for n in PHONEMES]
    mels, info = e.generate_stream(ids, st, slots=2, want_info=True, **STOP_AT_MIN)      # computed once, never changed
    return e, ids, st, mels, info


def test_against_its_own_mels_the_distance_is_zero(world):
    from kokoro.inference.evaluate import evaluate
    e, ids, st, mels, info = world
    durs = [d.clone() for d in info["durations"]]
    recs, summ = evaluate(e, ids, st, mels, slots=2, durations=durs, names=list("abcd"), **STOP_AT_MIN)
    assert [r["name"] for r in recs] == list("abcd") and len({r["frames"] for r in recs}) >= 2
    for r, m, b in zip(recs, mels, info["bounds"]):
        assert r["frames"] == r["ref_frames"] == m.shape[0] == b[0] + 1 < b[2]
        assert r["mcd_dtw"] == 0.0 and r["mel_l1_dtw"] == 0.0 and r["len_ratio"] == 1.0 and r["dur_abs_err"] == 0.0
        assert r["hit_bound"] is False
    assert summ["utterances"] == 4 and summ["hit_bound_share"] == 0.0
    assert summ["mcd_dtw"] == {"mean": 0.0, "median": 0.0, "p95": 0.0} and summ["len_ratio"] == {"mean": 1.0, "median": 1.0, "p95": 1.0}


def test_against_frame_doubled_copies_the_distance_is_zero_at_half_the_length(world):
    from kokoro.inference.evaluate import evaluate
    e, ids, st, mels, _ = world
    recs, summ = evaluate(e, ids, st, [m.repeat_interleave(2, dim=0) for m in mels], slots=2, **STOP_AT_MIN)
    for r, m in zip(recs, mels):
        assert r["mcd_dtw"] == 0.0 and r["mel_l1_dtw"] == 0.0 and r["len_ratio"] == 0.5
        assert r["ref_frames"] == 2 * r["frames"] == 2 * m.shape[0] and "dur_abs_err" not in r
    assert summ["len_ratio"]["mean"] == 0.5 and "dur_abs_err" not in summ


def test_stream_and_batches_give_the_same_records(world):
    """generate_stream documents its mels within 1e-4 of generate_batch's.  On one path that moves the aligned mel L1 by at most
    1e-4 and a frame's cepstral distance by at most sqrt(M) 1e-4 (the K rows of the DCT are orthonormal: the projection does not
    lengthen a difference), so mcd_dtw by at most (10 / ln 10) sqrt(2) sqrt(M) 1e-4; the references are warped noisy copies, whose
    alignment no 1e-4 moves."""
    from kokoro.inference.evaluate import evaluate
    e, ids, st, mels, info = world
    g = torch.Generator().manual_seed(3)
    refs = []
    for m in mels:
        idx = torch.linspace(0, m.shape[0] - 1, int(1.3 * m.shape[0]) + 1).round().long()
        refs.append(m.cpu()[idx] + 0.05 * torch.randn(idx.numel(), m.shape[1], generator=g))
    durs = [d + 1 for d in info["durations"]]
    a, sa = evaluate(e, ids, st, refs, stream=True, slots=3, durations=durs, **STOP_AT_MIN)
    b, sb = evaluate(e, ids, st, refs, stream=False, batch_size=3, durations=durs, **STOP_AT_MIN)
    M = mels[0].shape[1]
    for x, y, n in zip(a, b, PHONEMES):
        assert {k: x[k] for k in ("name", "frames", "ref_frames", "len_ratio", "hit_bound", "dur_abs_err")} == \
               {k: y[k] for k in ("name", "frames", "ref_frames", "len_ratio", "hit_bound", "dur_abs_err")}
        assert x["dur_abs_err"] == n and 0.0 < x["mcd_dtw"] and 0.0 < x["mel_l1_dtw"] < 0.2
        print(f"{n} phonemes: mcd_dtw {x['mcd_dtw']!r} / {y['mcd_dtw']!r}  mel_l1_dtw {x['mel_l1_dtw']!r} / {y['mel_l1_dtw']!r}")
        assert abs(x["mel_l1_dtw"] - y["mel_l1_dtw"]) <= 1e-4
        assert abs(x["mcd_dtw"] - y["mcd_dtw"]) <= 10 / math.log(10) * math.sqrt(2) * math.sqrt(M) * 1e-4
    assert sa["utterances"] == sb["utterances"] == 4 and abs(sa["mcd_dtw"]["mean"] - sb["mcd_dtw"]["mean"]) <= 10 / math.log(10) * math.sqrt(2 * M) * 1e-4


@pytest.mark.parametrize("stream", [False, True])
def test_a_cap_below_the_minimum_length_cuts_every_row(world, stream):
    """max_len_cap = 8 lies below every row's minimum length (floor 12), so each row's bound is its minimum + 1 and the row ends there
    before the stop rule is asked (slot_frames keeps the stream's slots long enough for the predicted lengths)."""
    from kokoro.inference.evaluate import evaluate
    e, ids, st, mels, info = world
    kw = dict(slot_frames=200) if stream else {}
    recs, summ = evaluate(e, ids, st, mels, stream=stream, slots=2, batch_size=4, max_len_cap=8, **kw, **STOP_AT_MIN)
    assert all(r["hit_bound"] is True for r in recs) and summ["hit_bound_share"] == 1.0
    assert [r["frames"] for r in recs] == [b[0] + 1 for b in info["bounds"]]
