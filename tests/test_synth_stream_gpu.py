"""GPU suite, engine level: KokoroEngine.generate_stream (continuous batching).  Every mel must be what generate_batch gives that
utterance alone, whatever the slot count, the admission order and the previous occupant of its slot."""
import os

import numpy as np
import pytest
import torch

from oracle import kokoro_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = "duration_adaptor.variance_adaptor"
BASE, EXTRA = (2, 9, 23, 40, 64), (5, 31)   # the utterances of test_synth_gpu.py (T_b = 32, 96, 216, 507, 545 frames) and two more
ORDER = (2, 0, 4, 1, 3, 5, 6)          # 23, 2, 64, 9, 40, 5, 31 phonemes; with slots = 2 the later ones are admitted into used slots
DUR_BIAS = 2.7                         # durations ~ e^2.7 per phoneme: the 64-phoneme row has more than 512 frames
SETTINGS = {"min": dict(max_len=160, stop_threshold=0.0), "max": dict(max_len=160, stop_threshold=2.0, post_expected_stop_threshold=2.0),
            "defaults": dict(max_len=160)}                     # (the three stop settings of test_synth_gpu.py)


def _fixture():                        # (the model of test_synth_gpu.py)
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


def _engine(d, P, mode="f32"):
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode=mode, init=False, total_steps=100)
    e.load_params(P)
    return e


def _utterances(d):
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g) for n in BASE]
    st = [torch.randint(0, 3, (n,), generator=g) for n in BASE]
    ids += [torch.randint(1, d.vocab, (n,), generator=g) for n in EXTRA]
    st += [torch.randint(0, 3, (n,), generator=g) for n in EXTRA]
    return [ids[i].cuda() for i in ORDER], [st[i].cuda() for i in ORDER]


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d, P = _fixture()
    e = _engine(d, P)
    ids, st = _utterances(d)
    alone = {}                         # setting -> [(mel, durations, T)] of generate_batch([u]): computed once, never changed

    def ref(setting):
        if setting not in alone:
            rows = []
            for u, s in zip(ids, st):
                m, info = e.generate_batch([u], [s], want_info=True, **SETTINGS[setting])
                rows.append((m[0], info["durations"][0], info["T"][0], info["bounds"][0]))
            alone[setting] = rows
        return alone[setting]
    return e, ids, st, ref


def _check(mels, info, rows, order):
    assert len(mels) == len(order)
    for k, i in enumerate(order):
        mel, dur, T, bounds = rows[i]
        assert torch.equal(info["durations"][k], dur), f"utterance {i}: durations"
        assert info["T"][k] == T and tuple(info["bounds"][k]) == tuple(bounds)
        assert mels[k].shape == mel.shape, f"utterance {i}: {mels[k].shape[0]} frames, alone {mel.shape[0]}"
        assert bool(torch.isfinite(mels[k]).all())
        torch.testing.assert_close(mels[k], mel, atol=1e-4, rtol=0)


@pytest.mark.parametrize("slots,reverse", [(2, False), (1, False), (8, False), (2, True)])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_stream_rows_equal_generate_batch_alone(world, setting, slots, reverse):
    e, ids, st, ref = world
    rows = ref(setting)
    assert max(r[2] for r in rows) > 512, "one row runs the chunked GroupNorm"
    order = list(range(len(ids)))[::-1] if reverse else list(range(len(ids)))
    mels, info = e.generate_stream([ids[i] for i in order], [st[i] for i in order], slots=slots, want_info=True, **SETTINGS[setting])
    _check(mels, info, rows, order)
    if setting == "min":
        assert len({m.shape[0] for m in mels}) >= 3, "rows of different lengths"


def test_stream_without_stress_and_want_info_off(world):
    e, ids, st, ref = world
    kw = SETTINGS["min"]
    mels = e.generate_stream(ids[:3], None, slots=2, **kw)
    for u, m in zip(ids[:3], mels):
        one = e.generate_batch([u], **kw)[0]
        assert m.shape == one.shape
        torch.testing.assert_close(m, one, atol=1e-4, rtol=0)
    assert e.generate_stream([], slots=2) == [] and e.generate_stream([], want_info=True) == e.generate_batch([], want_info=True)


def test_stream_ignores_stale_self_attention_caches(world):
    """NaN in every self-attention cache before the call: nothing past klen is read, and a refilled slot does not see its
    previous occupant."""
    e, ids, st, ref = world
    kw = dict(slots=2, slot_frames=600, **SETTINGS["max"])
    a = e.generate_stream(ids, st, **kw)
    for i in range(e.dims.dec_layers):
        for c in ("kcache", "vcache"):
            e._buf(f"str.dec{i}.{c}", 2, 600, e.dims.hidden, dtype=e.dec_dt).fill_(float("nan"))
    b, info = e.generate_stream(ids, st, want_info=True, **kw)
    for x, y in zip(a, b):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)
    _check(b, info, ref("max"), list(range(len(ids))))


def test_stream_replay_equals_eager(world):
    e, ids, st, ref = world
    kw = dict(slots=2, **SETTINGS["defaults"])
    a = e.generate_stream(ids, st, decode_graph=True, **kw)
    b = e.generate_stream(ids, st, decode_graph=False, **kw)
    c = e.generate_stream(ids, st, decode_graph=True, **kw)
    d = e.generate_stream(ids, st, decode_graph=True, check_every=5, **kw)
    for x, y, z, w in zip(a, b, c, d):
        assert torch.equal(x, y), "replay against eager"
        assert torch.equal(x, z), "a second identical call"
        assert torch.equal(x, w), "check_every"


def test_stream_errors(world):
    e, ids, st, ref = world
    Ts = [r[2] for r in ref("max")]
    first = next(i for i, t in enumerate(Ts) if t > 150)
    with pytest.raises(ValueError, match=f"utterance {first}:"):
        e.generate_stream(ids, st, slots=2, slot_frames=150, **SETTINGS["max"])
    with pytest.raises(ValueError):
        e.generate_stream(ids[:2], [st[0], None])
    with pytest.raises(ValueError, match="empty utterance"):
        e.generate_stream([ids[0], ids[1][:0]], None)
    with pytest.raises(ValueError):
        e.generate_stream(ids[:2], st[:1])
    mels = e.generate_stream(ids[:2], st[:2], slots=2, **SETTINGS["min"])        # and the engine still works
    assert [m.shape for m in mels] == [r[0].shape for r in ref("min")[:2]]


def test_stream_bf16_mode():
    """bf16 storage under the bound of test_generate_batch_bf16_mode: stop head disabled, each row close to the bf16 batch path on
    that utterance alone."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d, P = _fixture()
    e = _engine(d, P, "bf16")
    ids, st = _utterances(d)
    kw = dict(max_len=20, stop_threshold=2.0, post_expected_stop_threshold=2.0)
    mels = e.generate_stream(ids, st, slots=3, **kw)
    for b, (u, s) in enumerate(zip(ids, st)):
        one = e.generate_batch([u], [s], **kw)[0]
        assert mels[b].shape == one.shape and bool(torch.isfinite(mels[b]).all())
        assert float((mels[b] - one).abs().max()) <= 0.05 * max(1.0, float(one.abs().max())), f"row {b}"
