"""GPU suite: the pronunciation scores of kokoro.inference.evaluate.evaluate on the tiny random-weight engine of test_evaluate_gpu.py:
the documented keys and no others, their values against PhoneAligner.score called directly on the same mels, the reference side, the
gaps, an infeasible side, and the call without a phone model, which launches and returns what it did before."""
import os

import numpy as np
import pytest
import torch

from oracle import kokoro_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = "duration_adaptor.variance_adaptor"
PHONEMES = (2, 9, 5, 23)
DUR_BIAS = 1.5
STOP_AT_MIN = dict(max_len=160, stop_threshold=0.0)       # the stop rule fires on the first frame it may: at the row's minimum length
SYN_KEYS = ("gop", "logpost", "phone_acc", "gop_min", "gop_min_token")
REF_KEYS = ("ref_gop", "ref_logpost", "ref_phone_acc")
NEW_KEYS = SYN_KEYS + REF_KEYS + ("gop_gap", "phone_acc_gap")


def _fixture():                        # (the tiny model of test_evaluate_gpu.py)
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
    from kokoro.inference.evaluate import evaluate
    from kokoro_ruslan_amd import lib as kk
    from kokoro_ruslan_amd.align import PhoneAligner
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d, P = _fixture()
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g).cuda() for n in PHONEMES]
    st = [torch.randint(0, 3, (n,), generator=g).cuda() for n in PHONEMES]
    mels, info = e.generate_stream(ids, st, slots=2, want_info=True, **STOP_AT_MIN)      # what evaluate(slots=2) synthesizes again
    refs = []
    for m in mels:                     # references a fifth longer: warped noisy copies
        idx = torch.linspace(0, m.shape[0] - 1, int(1.2 * m.shape[0]) + 1).round().long()
        refs.append(m.cpu()[idx] + 0.05 * torch.randn(idx.numel(), m.shape[1], generator=g))
    durs = [x.clone() for x in info["durations"]]
    kw = dict(slots=2, durations=durs, names=list("abcd"), **STOP_AT_MIN)
    evaluate(e, ids, st, refs, **kw)                                     # (whatever a first call sets up is set up)
    n0 = kk.launches
    plain, plain_summary = evaluate(e, ids, st, refs, **kw)              # before anything of the phone models has run
    plain_launches = kk.launches - n0
    al = PhoneAligner(n_classes=d.vocab)
    model, _, _ = al.fit(refs, [i.cpu() for i in ids], iters=2)          # a phone model of the "recordings"
    return dict(e=e, ids=ids, st=st, mels=mels, refs=refs, kw=kw, plain=plain, plain_summary=plain_summary, plain_launches=plain_launches,
                al=al, model=model, evaluate=evaluate, kk=kk)


def test_a_phone_model_adds_exactly_the_documented_keys_with_the_values_of_a_direct_score(world):
    w = world
    recs, summ = w["evaluate"](w["e"], w["ids"], w["st"], w["refs"], phone_model=w["model"], **w["kw"])
    syn = w["al"].score(w["mels"], w["ids"], (), w["model"])
    ref = w["al"].score(w["refs"], w["ids"], (), w["model"])
    for r, q, s, x in zip(recs, w["plain"], syn, ref):
        assert set(r) == set(q) | set(NEW_KEYS) and not set(q) & set(NEW_KEYS)
        assert {k: r[k] for k in q} == q, "the other fields are what they are without a phone model"
        assert s["feasible"] and x["feasible"]
        assert {k: r[k] for k in SYN_KEYS} == {k: s[k] for k in SYN_KEYS}
        assert {k: r[k] for k in REF_KEYS} == {"ref_" + k: x[k] for k in ("gop", "logpost", "phone_acc")}
        assert r["gop_gap"] == s["gop"] - x["gop"] and r["phone_acc_gap"] == s["phone_acc"] - x["phone_acc"]
        assert r["gop"] <= 0.0 and r["logpost"] <= r["gop"] + 1e-12 and 0.0 <= r["phone_acc"] <= 1.0 and r["gop_min"] <= r["gop"] + 1e-12
        assert isinstance(r["gop_min_token"], int) and 0 <= r["gop_min_token"] < len(s["tokens"]["frames"])
    assert set(summ) == set(w["plain_summary"]) | {"pron_infeasible"} | (set(NEW_KEYS) - {"gop_min_token"})
    assert summ["pron_infeasible"] == 0
    gaps = torch.tensor([r["gop_gap"] for r in recs], dtype=torch.float64)
    assert summ["gop_gap"]["mean"] == float(gaps.mean()) and {k: summ[k] for k in w["plain_summary"]} == w["plain_summary"]


def test_a_given_aligner_and_optional_ids_are_used_and_an_infeasible_side_gets_none(world):
    w = world
    calls = []

    class Spy:
        def score(self, mels, ids, optional_ids=(), model=None, feats=None):
            calls.append((len(mels), tuple(optional_ids), model is w["model"]))
            return w["al"].score(mels, ids, optional_ids, model, feats)
    short = list(w["refs"])
    short[3] = short[3][:PHONEMES[3] - 1]                                 # 23 phonemes on 22 frames: the recording cannot be aligned
    recs, summ = w["evaluate"](w["e"], w["ids"], w["st"], short, phone_model=w["model"], phone_aligner=Spy(), optional_ids=(0,), **w["kw"])
    assert calls == [(4, (0,), True), (4, (0,), True)], "one score call for the synthesis and one for the recordings"
    r = recs[3]
    assert r["ref_gop"] is None and r["ref_logpost"] is None and r["ref_phone_acc"] is None and r["gop_gap"] is None and r["phone_acc_gap"] is None
    assert r["gop"] is not None and all(q["gop_gap"] is not None for q in recs[:3])
    assert summ["pron_infeasible"] == 1
    for bad in (dict(phone_aligner=Spy()), dict(optional_ids=(0,))):
        with pytest.raises(ValueError, match="need a phone_model"):
            w["evaluate"](w["e"], w["ids"], w["st"], w["refs"], **bad, **w["kw"])


def test_without_a_phone_model_records_and_launches_are_what_they_were(world):
    """The fixture's call was made before any phone model existed; this one after every other test of the file may have run."""
    w = world
    n0 = w["kk"].launches
    recs, summ = w["evaluate"](w["e"], w["ids"], w["st"], w["refs"], **w["kw"])
    assert w["kk"].launches - n0 == w["plain_launches"], "no launch more than before"
    assert [set(r) for r in recs] == [set(q) for q in w["plain"]] and recs == w["plain"] and summ == w["plain_summary"]
    assert not set(NEW_KEYS) & set(recs[0]) and "pron_infeasible" not in summ
