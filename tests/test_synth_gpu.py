"""GPU suite, engine level: KokoroEngine.generate_batch.  Row b of a ragged batch must equal the reference's B = 1
forward_inference on utterance b alone — the oracle's generate (pinned to the reference by inference_tiny.npz) run at B = 1."""
import os

import numpy as np
import pytest
import torch

from oracle import kokoro_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = "duration_adaptor.variance_adaptor"
SIZES = (2, 9, 23, 40, 64)
DUR_BIAS = 2.7          # durations ~ e^2.7: T_b = 32, 96, 216, 507, 545 frames (the last one spans two GroupNorm chunks)


def _fixture():
    fx = np.load(os.path.join(GOLDEN, "inference_tiny.npz"))
    d = O.ModelDims(*[int(x) for x in fx["dims"]])
    seed = int(fx["seed"])
    P = O.init_params(d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in P.items():
        if p.dim() == 1:
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return fx, d, P


def _engine(d, P, mode="f32"):
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode=mode, init=False, total_steps=100)
    e.load_params(P)
    return e


def _utterances(d):
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g) for n in SIZES]
    st = [torch.randint(0, 3, (n,), generator=g) for n in SIZES]
    return ids, st


@pytest.fixture(scope="module")
def ragged():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    fx, d, P = _fixture()
    P[f"{VA}.duration_predictor.linear.bias"].fill_(DUR_BIAS)
    return d, P, _engine(d, P), _utterances(d)


SETTINGS = {"min": dict(max_len=160, stop_threshold=0.0), "max": dict(max_len=160, stop_threshold=2.0, post_expected_stop_threshold=2.0), "defaults": dict(max_len=160)}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_generate_batch_rows_equal_the_oracle_alone(ragged, setting):
    d, P, e, (ids, st) = ragged
    kw = SETTINGS[setting]
    mels, info = e.generate_batch([u.cuda() for u in ids], [s.cuda() for s in st], want_info=True, **kw)
    assert len(mels) == len(ids)
    assert max(info["T"]) > 512, "one row runs the chunked GroupNorm"
    Bf = O.make_buffers(d)
    counts = []
    for b, (u, s) in enumerate(zip(ids, st)):
        ref, rinfo = O.generate(P, Bf, u[None], s[None], d, want=True, **kw)
        assert torch.equal(info["durations"][b].cpu(), rinfo["durations"][0]), f"row {b}: durations"
        assert tuple(info["bounds"][b]) == tuple(rinfo["bounds"]), f"row {b}: bounds"
        assert info["T"][b] == rinfo["bounds"][1]
        assert tuple(mels[b].shape) == tuple(ref.shape[1:]), f"row {b}: same stop decision"
        torch.testing.assert_close(mels[b].cpu(), ref[0], atol=1e-4, rtol=0)
        counts.append(mels[b].shape[0])
    if setting == "min":
        assert counts == [lo + 1 if lo + 1 < hi else hi for lo, _, hi in info["bounds"]]
        assert len({c for c in counts if c > 13}) >= 3, counts
    if setting == "max":
        assert counts == [hi for _, _, hi in info["bounds"]]


def test_generate_batch_rows_equal_generate_alone(ragged):
    d, P, e, (ids, st) = ragged
    kw = dict(max_len=60, stop_threshold=0.0)
    mels = e.generate_batch([u.cuda() for u in ids], [s.cuda() for s in st], **kw)
    for b, (u, s) in enumerate(zip(ids, st)):
        one = e.generate(u[None].cuda(), s[None].cuda(), **kw)[0]
        assert one.shape == mels[b].shape
        torch.testing.assert_close(mels[b], one, atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["never_stops", "stops_at_min_length"])
def test_generate_batch_of_one_matches_the_reference(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    fx, d, P = _fixture()
    e = _engine(d, P)
    ids = torch.from_numpy(fx[f"{name}/ids"])
    max_len, thr = fx[f"{name}/kw"]
    ref = torch.from_numpy(fx[f"{name}/mel"])[0]
    e.train_dropout = True
    mel = e.generate_batch([ids[0].cuda()], max_len=int(max_len), stop_threshold=float(thr))[0].cpu()
    assert e.train_dropout is True, "dropout off inside, flag restored"
    assert mel.shape == ref.shape
    torch.testing.assert_close(mel, ref, atol=1e-4, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_generate_batch_replay_equals_eager(mode):
    """Frame counts and values do not depend on check_every or on the decode graph (default model size, ragged batch)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=3)
    g = torch.Generator().manual_seed(1)
    ids = [torch.randint(1, 59, (n,), generator=g).cuda() for n in (40, 7, 25)]
    kw = dict(max_len=90, stop_threshold=0.0, min_len_ratio=0.5, min_len_floor=1)
    a = e.generate_batch(ids, decode_graph=False, check_every=1, **kw)
    tol = 1e-3 if mode == "f32" else 0.05
    for ce in (1, 7, 16):
        b = e.generate_batch(ids, decode_graph=True, check_every=ce, **kw)
        for x, y in zip(a, b):
            assert x.shape == y.shape and bool(torch.isfinite(x).all())
            assert float((x - y).abs().max()) <= tol * max(1.0, float(x.abs().max()))


def test_generate_batch_bf16_mode():
    """bf16 storage: with the stop head disabled, the oracle's frame counts; each row close to bf16 generate() on that utterance
    alone; and the fixture's two utterances within the bf16 inference bound of test_inference.py against the oracle."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    fx, d, P = _fixture()
    e = _engine(d, P, "bf16")
    ids, st = _utterances(d)
    kw = dict(max_len=20, stop_threshold=2.0, post_expected_stop_threshold=2.0)
    mels = e.generate_batch([u.cuda() for u in ids], [s.cuda() for s in st], **kw)
    Bf = O.make_buffers(d)
    for b, (u, s) in enumerate(zip(ids, st)):
        ref = O.generate(P, Bf, u[None], s[None], d, **kw)[0]
        one = e.generate(u[None].cuda(), s[None].cuda(), **kw)[0].cpu()
        mel = mels[b].cpu()
        assert mel.shape == ref.shape == one.shape and bool(torch.isfinite(mel).all())
        assert float((mel - one).abs().max()) <= 0.05 * max(1.0, float(one.abs().max())), f"row {b}"
    ids2, st2 = torch.from_numpy(fx["batch2_padded_stress/ids"]), torch.from_numpy(fx["batch2_padded_stress/stress"])
    rows = [ids2[b][ids2[b] != 0] for b in range(2)]
    srows = [st2[b][:len(rows[b])] for b in range(2)]
    kw = dict(max_len=10, stop_threshold=2.0, post_expected_stop_threshold=2.0)
    mels = e.generate_batch([r.cuda() for r in rows], [s_.cuda() for s_ in srows], **kw)
    for b in range(2):
        ref = O.generate(P, Bf, rows[b][None], srows[b][None], d, **kw)[0]
        mel = mels[b].cpu()
        assert mel.shape == ref.shape
        assert float((mel - ref).abs().mean()) < 0.08 * float(ref.abs().mean()) + 0.02, f"row {b}"


def test_generate_batch_rejects_mixed_stress():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    fx, d, P = _fixture()
    e = _engine(d, P)
    ids, st = _utterances(d)
    with pytest.raises(ValueError):
        e.generate_batch([u.cuda() for u in ids[:2]], [st[0].cuda(), None])
