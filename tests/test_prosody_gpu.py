"""GPU suite, engine level: prosody controls in KokoroEngine.generate / generate_batch / generate_stream against the oracle's
variance adaptor restated with the same controls (tests/prosody_oracle.py), one utterance at a time at B = 1.

The comparisons of durations and bucket indices are exact, so the oracle's own values must keep clear of the rounding and bin
boundaries; that is asserted here (not skipped): every d and d / speed at least 1e-3 from k + 0.5, every controlled pitch / energy of
a live frame at least 1e-4 from a bin edge (exact zeros aside) and every raw pitch at least 1e-4 from 0, the voiced / unvoiced
switch.  Both margins are far above the fp32 distance between engine and oracle that the duration-equality tests of
test_synth_gpu.py already rely on."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prosody_oracle as PO  # noqa: E402
from kokoro_ruslan_amd.prosody import Prosody  # noqa: E402
from oracle import kokoro_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = PO.VA
SIZES = (2, 9, 23)
DUR_BIAS = 2.0
KW = dict(max_len=60, stop_threshold=0.0)       # every row stops one frame past its minimum length: a few dozen frames
NAN = math.nan


def fixture_model():
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


def utterances(d):
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g) for n in SIZES]
    st = [torch.randint(0, 3, (n,), generator=g) for n in SIZES]
    return ids, st


def speed_controls():
    """name -> one Prosody per utterance"""
    g = torch.Generator().manual_seed(SPEED_SEED)
    return {"slow": [Prosody(speed=0.5)] * 3, "fast": [Prosody(speed=1.6)] * 3,
            "per-phoneme": [Prosody(speed=(0.5 + 2.0 * torch.rand(n, generator=g)).tolist()) for n in SIZES]}


def variance_controls():
    """Scale, shift and forced per-phoneme values at once, per utterance: every third phoneme's pitch and every fourth's energy are
    forced, the others scaled and shifted.  The scales keep the results inside (0, 1): a value the clamp puts on 1 sits on a bin edge."""
    out = []
    for k, n in enumerate(SIZES):
        g = torch.Generator().manual_seed(VARIANCE_SEED + k)
        fp, fe = [NAN] * n, [NAN] * n
        for j in range(0, n, 3):
            fp[j] = 0.33
        for j in range(1, n, 4):
            fe[j] = 0.61
        out.append(Prosody(pitch_scale=(0.3 + 0.4 * torch.rand(n, generator=g)).tolist(), pitch_shift=0.2, energy_scale=0.4,
                           energy_shift=(0.05 + 0.3 * torch.rand(n, generator=g)).tolist(), pitch=fp, energy=fe))
    return out


def mixed_controls():
    """A different Prosody per row, every kind of control among them."""
    return [Prosody(speed=0.5, energy_scale=0.4, energy_shift=0.1),
            Prosody(durations=[3, 0, 5, -1, 2, -1, -1, 0, 4], pitch=[0.33, NAN, NAN, 0.9, NAN, NAN, 0.05, NAN, NAN]),
            Prosody(speed=1.6, pitch_scale=0.5, pitch_shift=0.2, energy=[0.61 if j % 2 else NAN for j in range(23)])]


SPEED_SEED, VARIANCE_SEED = 1, 300      # (chosen on the host so that the oracle's values meet the preconditions asserted below)
FORCED = [[2, 2], [3, 0, 5, -1, 2, -1, -1, 0, 4], [-1] * 10 + [0, 1, 4] + [-1] * 10]


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d, P = fixture_model()
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    ids, st = utterances(d)
    return d, P, O.make_buffers(d), e, ids, st


def _cuda(xs):
    return [x.cuda() for x in xs]


def _oracle_rows(monkeypatch, world, prosody):
    d, P, Bf, e, ids, st = world
    return [PO.generate(monkeypatch, P, Bf, u[None], s[None], d, [prosody[b]], **KW) for b, (u, s) in enumerate(zip(ids, st))]


def _check_rows(mels, info, refs, exact_T=True):
    for b, (ref, rinfo) in enumerate(refs):
        assert torch.equal(info["durations"][b].cpu(), rinfo["durations"][0]), f"row {b}: durations"
        assert tuple(info["bounds"][b]) == tuple(rinfo["bounds"]), f"row {b}: bounds"
        assert info["T"][b] == rinfo["bounds"][1] == max(int(rinfo["durations"].sum()), 3), f"row {b}: T"
        assert tuple(mels[b].shape) == tuple(ref.shape[1:]), f"row {b}: same stop decision"
        torch.testing.assert_close(mels[b].cpu(), ref[0], atol=1e-4, rtol=0)


# ---- 1. no controls given ---------------------------------------------------------------------------------------------------------

def test_neutral_prosody_equals_none_in_all_three_entry_points(world):
    d, P, Bf, e, ids, st = world
    a, ia = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, **KW)
    for pr in (Prosody(), [Prosody(), None, Prosody(speed=[1.0] * 23, durations=[-1] * 23, pitch=[NAN] * 23)]):
        b, ib = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, prosody=pr, **KW)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(ia["durations"], ib["durations"]))
        assert ia["T"] == ib["T"] and ia["bounds"] == ib["bounds"]
    a, ia = e.generate_stream(_cuda(ids), _cuda(st), slots=2, want_info=True, **KW)
    b, ib = e.generate_stream(_cuda(ids), _cuda(st), slots=2, want_info=True, prosody=Prosody(), **KW)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(ia["durations"], ib["durations"]))
    assert ia["T"] == ib["T"] and ia["bounds"] == ib["bounds"]
    pad = torch.zeros(2, 9, dtype=torch.int64)                    # generate: a padded batch, pads included
    pad[0], pad[1, :2] = ids[1], ids[0]
    a = e.generate(pad.cuda(), None, **KW)
    b = e.generate(pad.cuda(), None, prosody=Prosody(), **KW)
    c = e.generate(pad.cuda(), None, prosody=[None, Prosody()], **KW)
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- 2. speed ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["slow", "fast", "per-phoneme"])
def test_speed(world, monkeypatch, name):
    d, P, Bf, e, ids, st = world
    prosody = speed_controls()[name]
    refs = _oracle_rows(monkeypatch, world, prosody)
    for b, (_, rinfo) in enumerate(refs):
        m = PO.half_margin(rinfo["d"], rinfo["speed"])
        print(f"{name} row {b}: margin of d and d / speed from a half {m:.5f}, durations {rinfo['durations'][0].tolist()}")
        assert m >= 1e-3, "precondition: pick another seed or speed"
    mels, info = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, prosody=prosody, **KW)
    _check_rows(mels, info, refs)
    base = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, **KW)[1]
    if name == "slow":
        assert all(int(x.sum()) > int(y.sum()) for x, y in zip(info["durations"][1:], base["durations"][1:]))
    for x, y in zip(info["durations"], base["durations"]):
        assert torch.equal(x == 0, y == 0), "no phoneme appears or vanishes with the speed"
    one = e.generate(ids[1][None].cuda(), st[1][None].cuda(), prosody=prosody[1], **KW)[0]       # generate at B = 1: the same row
    assert one.shape == mels[1].shape
    torch.testing.assert_close(one.cpu(), refs[1][0][0], atol=1e-4, rtol=0)


# ---- 3. forced durations ------------------------------------------------------------------------------------------------------------

def test_forced_durations(world, monkeypatch):
    d, P, Bf, e, ids, st = world
    prosody = [Prosody(durations=f) for f in FORCED]
    refs = _oracle_rows(monkeypatch, world, prosody)
    for b, (_, rinfo) in enumerate(refs):
        assert PO.half_margin(rinfo["d"], rinfo["speed"]) >= 1e-3
    mels, info = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, prosody=prosody, **KW)
    _check_rows(mels, info, refs)
    base = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, **KW)[1]
    for b, f in enumerate(FORCED):
        f = torch.tensor(f)
        got = info["durations"][b].cpu()
        assert torch.equal(got[f >= 0], f[f >= 0]), "forced values are used as given"
        assert torch.equal(got[f < 0], base["durations"][b].cpu()[f < 0]), "-1 keeps the model's"
        assert info["T"][b] == max(int(got.sum()), 3)
    assert info["T"][0] == 4 and info["T"][1] == 3 + 5 + 2 + 4 + int(base["durations"][1][[3, 5, 6]].sum())


def test_row_forced_to_all_zeros_decodes_as_a_three_frame_row(world):
    """Nothing of the text reaches the decoder then (every frame of the memory is masked), so the row must equal, bit for bit, what
    the same engine gives today when the MODEL predicts all zeros: the same weights with the duration bias at -10."""
    d, P, Bf, e, ids, st = world
    mels, info = e.generate_batch(_cuda(ids[:2]), _cuda(st[:2]), want_info=True, prosody=[None, Prosody(durations=[0] * 9)], **KW)
    assert info["durations"][1].tolist() == [0] * 9 and info["T"][1] == 3
    assert tuple(info["bounds"][1]) == tuple(e._generation_bounds(3, 60, 0.7, 12, 3.0, 1600))
    P0 = {k: v.clone() for k, v in P.items()}
    P0[f"{VA}.duration_predictor.linear.bias"].fill_(-10.0)
    try:
        e.load_params(P0)
        ref, rinfo = e.generate_batch(_cuda(ids[1:2]), _cuda(st[1:2]), want_info=True, **KW)
    finally:
        e.load_params(P)
    assert rinfo["durations"][0].tolist() == [0] * 9 and rinfo["T"] == [3] and rinfo["bounds"][0] == info["bounds"][1]
    assert mels[1].shape == ref[0].shape
    assert torch.equal(torch.isnan(mels[1]), torch.isnan(ref[0])) and torch.equal(torch.nan_to_num(mels[1]), torch.nan_to_num(ref[0]))


# ---- 4. pitch and energy ------------------------------------------------------------------------------------------------------------

def test_pitch_and_energy_controls(world, monkeypatch):
    d, P, Bf, e, ids, st = world
    prosody = variance_controls()
    refs = _oracle_rows(monkeypatch, world, prosody)
    changed = 0
    for b, (_, r) in enumerate(refs):
        live = r["live"]
        mp = PO.bin_margin(r["pitch_c"], live, Bf[f"{VA}.pitch_bins"])
        me = PO.bin_margin(r["energy_c"], live, Bf[f"{VA}.energy_bins"])
        m0 = float(r["pitch"][live].abs().min())
        print(f"row {b}: margins from a bin edge: pitch {mp:.6f} energy {me:.6f}; raw pitch from 0: {m0:.6f}")
        assert mp >= 1e-4 and me >= 1e-4 and m0 >= 1e-4, "precondition: pick another seed or control value"
        assert PO.half_margin(r["d"], r["speed"]) >= 1e-3
        changed += int((r["pidx"] != torch.bucketize(r["pitch"].clamp(0, 1), Bf[f"{VA}.pitch_bins"]))[live].sum())
        changed += int((r["eidx"] != torch.bucketize(r["energy"].clamp(0, 1), Bf[f"{VA}.energy_bins"]))[live].sum())
    assert changed > 50, "the controls move the buckets"
    for b, (u, s) in enumerate(zip(ids, st)):                     # alone, so that the buckets of the row sit in syn.va.* after the call
        mels, info = e.generate_batch([u.cuda()], [s.cuda()], want_info=True, prosody=[prosody[b]], **KW)
        ref, r = refs[b]
        T = info["T"][0]
        n = int(r["durations"].sum())
        pidx, eidx = e._buf("syn.va.pidx", 1, T, dtype=torch.int32), e._buf("syn.va.eidx", 1, T, dtype=torch.int32)
        assert torch.equal(pidx[0, :n].cpu().long(), r["pidx"][0, :n]), f"row {b}: pitch buckets"
        assert torch.equal(eidx[0, :n].cpu().long(), r["eidx"][0, :n]), f"row {b}: energy buckets"
        _check_rows(mels, info, [refs[b]])


# ---- 5. rows alone ------------------------------------------------------------------------------------------------------------------

def test_rows_with_their_own_controls_equal_the_rows_alone(world):
    d, P, Bf, e, ids, st = world
    prosody = mixed_controls()
    alone = [e.generate_batch([u.cuda()], [s.cuda()], want_info=True, prosody=[prosody[b]], **KW) for b, (u, s) in enumerate(zip(ids, st))]
    mels, info = e.generate_batch(_cuda(ids), _cuda(st), want_info=True, prosody=prosody, **KW)
    smels, sinfo = e.generate_stream(_cuda(ids), _cuda(st), slots=2, want_info=True, prosody=prosody, **KW)     # the third row is a refill
    salone = [e.generate_stream([u.cuda()], [s.cuda()], slots=2, want_info=True, prosody=[prosody[b]], **KW) for b, (u, s) in enumerate(zip(ids, st))]
    for b in range(3):
        for (m, i), (am, ai) in (((mels, info), alone[b]), ((smels, sinfo), salone[b])):
            assert torch.equal(m[b], am[0]), f"row {b}"
            assert torch.equal(i["durations"][b], ai["durations"][0]) and i["T"][b] == ai["T"][0] and i["bounds"][b] == ai["bounds"][0]
        assert torch.equal(info["durations"][b], sinfo["durations"][b]) and info["bounds"][b] == sinfo["bounds"][b]
        torch.testing.assert_close(smels[b], mels[b], atol=1e-4, rtol=0)
    assert not torch.equal(info["durations"][0], e.generate_batch(_cuda(ids), _cuda(st), want_info=True, **KW)[1]["durations"][0])


# ---- 6. evaluation ------------------------------------------------------------------------------------------------------------------

def test_evaluate_on_forced_cache_durations_has_no_duration_error(world):
    from kokoro.inference.evaluate import evaluate
    d, P, Bf, e, ids, st = world
    g = torch.Generator().manual_seed(5)
    durs = [torch.randint(0, 4, (n,), generator=g) + 12 * (torch.arange(n) == 0) for n in SIZES]     # three synthetic cache entries
    refs = [torch.randn(int(x.sum()), d.mel, generator=g).cuda() for x in durs]
    for stream in (True, False):
        recs, summ = evaluate(e, _cuda(ids), _cuda(st), refs, stream=stream, slots=2, durations=durs,
                              prosody=[Prosody(durations=x) for x in durs], **KW)
        assert [r["dur_abs_err"] for r in recs] == [0.0, 0.0, 0.0] and summ["dur_abs_err"]["mean"] == 0.0
    recs, _ = evaluate(e, _cuda(ids), _cuda(st), refs, slots=2, durations=durs, **KW)
    assert any(r["dur_abs_err"] > 0 for r in recs), "without the controls the predictor's own error shows"
