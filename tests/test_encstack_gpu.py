"""GPU suite: the text-encoder forward as one persistent launch (kk_encoder_stack_fwd, csrc/kk_encstack.hip) against the
per-kernel sequence it replaces — every tensor the backward reads, for several batch shapes, both workgroup placements
(groups inside an XCD / groups spread over all XCDs: the hand-offs must not depend on it), dropout on and off — and under
load: hundreds of back-to-back graph replays beside the other branches of the step must give the same bits every time."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SAVED = ["sa.qkv_raw", "sa.qkv_n", "sa.ctx", "sa.lse", "xm", "ln2.y", "ln2.mean", "ln2.rstd", "ff.h1", "ff.g", "ff.f2", "ff.rstd_f", "xo"]


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import engine, spec, synthetic
    return engine, spec, synthetic


def _engine(mods, dims=None):
    engine, spec, _ = mods
    e = engine.KokoroEngine(dims or spec.ModelDims(), spec.StepHyper(gradient_accumulation_steps=1), math_mode="bf16",
                            total_steps=20000, seed=0)
    return e


def _encoder_tensors(e, B, P):
    """Clones of everything the encoder forward leaves behind for the backward (views of the workspace)."""
    d, out = e.dims, {}
    Ne, H, F, h = B * P, e.dims.hidden, e.dims.enc_ff, e.dims.heads
    shapes = {"sa.qkv_raw": (Ne, 3 * H), "sa.qkv_n": (Ne, 3 * H), "sa.ctx": (Ne, H), "sa.lse": (B, h, P), "xm": (Ne, H), "ln2.y": (Ne, H),
              "ln2.mean": (Ne,), "ln2.rstd": (Ne,), "ff.h1": (Ne, 2 * F), "ff.g": (Ne, F), "ff.f2": (Ne, H), "ff.rstd_f": (Ne,), "xo": (Ne, H)}
    f32 = {"sa.lse", "xm", "ln2.mean", "ln2.rstd", "ff.rstd_f", "xo"}
    for i in range(d.enc_layers):
        for k in SAVED:
            out[f"enc{i}.{k}"] = e._buf(f"enc{i}.{k}", *shapes[k], dtype=torch.float32 if k in f32 else e.enc_dt).clone()
        if i > 0:
            for k, shp, dt in ((".ln1.y", (Ne, H), e.enc_dt), (".ln1.mean", (Ne,), torch.float32), (".ln1.rstd", (Ne,), torch.float32)):
                out[f"enc{i}{k}"] = e._buf(f"enc{i}{k}", *shp, dtype=dt).clone()
    out["enc.norm.y"] = e._buf("enc.norm.y", Ne, H).clone()
    out["enc.norm.mean"], out["enc.norm.rstd"] = e._buf("enc.norm.mean", Ne).clone(), e._buf("enc.norm.rstd", Ne).clone()
    return out


def _forward(e, batch, fused, placement=0, seed=77):
    e.enc_fused, e.enc_placement = fused, placement
    e.rng.fill_(seed)
    out = e.forward_backward(batch, backward=False)
    torch.cuda.synchronize()
    B, P = batch["phoneme_indices"].shape
    return _encoder_tensors(e, B, P), out["losses"].clone()


def _rel(a, b):
    a, b = a.double(), b.double()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin)
    return float((a[fin] - b[fin]).norm() / (b[fin].norm() + 1e-30))


@pytest.mark.parametrize("B,T,P", [(8, 512, 64), (8, 256, 128), (8, 1024, 128), (3, 96, 50), (16, 128, 64), (2, 64, 33), (5, 160, 97)])
@pytest.mark.parametrize("dropout", [True, False])
def test_fused_encoder_matches_the_per_kernel_sequence(mods, B, T, P, dropout):
    _, _, synthetic = mods
    e = _engine(mods)
    assert e._encoder_stack_ok(B, P) == (B <= 8), "the engine takes the fused launch for up to 8 items (one per workgroup group)"
    e.enc_fused_max_batch = 64                           # (the launch itself serves any batch: a group walks its items in turn)
    assert e._encoder_stack_ok(B, P), "the shape must be served by the fused launch"
    e.train_dropout = dropout
    batch = {k: v.cuda() for k, v in synthetic.synthetic_batch(B, T, P, seed=5, ragged=B in (3, 5, 16)).items()}     # ragged: padded keys
    ref, ref_loss = _forward(e, batch, fused=False)
    for placement in (0, 1):
        got, loss = _forward(e, batch, fused=True, placement=placement)
        assert e.encoder_stack_error() == 0, "a group barrier of the fused encoder timed out"
        worst = []
        for name, r in ref.items():
            depth = e.dims.enc_layers if name.startswith("enc.norm") else int(name[3]) + 1
            err = _rel(got[name], r)
            # same arithmetic up to summation order inside a dot product; a flipped bf16 rounding is amplified layer by layer
            assert err < 6e-3 * depth, f"placement {placement}: {name} rel. error {err:.3e}"
            worst.append((err, name))
        # the dropout masks are the same functions of (seed, site, element): zeros in the same places
        g_ref, g_got = ref["enc0.ff.g"], got["enc0.ff.g"]
        same = float(((g_ref == 0) == (g_got == 0)).float().mean())
        assert same > 0.9999, f"GLU dropout masks differ ({same})"
        assert abs(float(loss[0]) - float(ref_loss[0])) < 2e-2 * abs(float(ref_loss[0])), (loss, ref_loss, max(worst))


def test_fused_encoder_first_layer_is_tight(mods):
    """Layer 0 sees identical inputs on both paths: differences are single bf16 roundings."""
    _, _, synthetic = mods
    e = _engine(mods)
    e.train_dropout = True
    batch = {k: v.cuda() for k, v in synthetic.synthetic_batch(8, 512, 64, seed=9).items()}
    ref, _ = _forward(e, batch, fused=False)
    got, _ = _forward(e, batch, fused=True)
    for k in ("sa.qkv_raw", "sa.qkv_n", "sa.ctx", "sa.lse", "xm", "ln2.y", "ff.h1", "ff.g", "ff.f2", "xo"):
        err = _rel(got["enc0." + k], ref["enc0." + k])
        assert err < 5e-3, f"enc0.{k}: {err:.3e}"
        if k == "sa.qkv_raw":      # the summation order differs, the values do not: almost all elements bit-equal
            eq = float((got["enc0." + k] == ref["enc0." + k]).float().mean())
            assert eq > 0.97, eq


def test_fused_encoder_is_deterministic_under_load(mods):
    """300 replays of the whole captured step (the decoder head and the gradient zero-fill run beside the encoder launch): with
    the seed pinned, the encoder's output must be bit-identical every time — a stale hand-off would show up as a difference."""
    _, _, synthetic = mods
    e = _engine(mods)
    e.train_dropout = True
    batch = {k: v.cuda() for k, v in synthetic.synthetic_batch(8, 512, 64, seed=11).items()}
    for placement in (0, 1):
        e.enc_placement = placement
        e._invalidate()
        g = None
        first = None
        for it in range(3):
            e.rng.fill_(123)
            e.forward_backward(batch, zero_grads=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        e.rng.fill_(123)
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            e.forward_backward(batch, zero_grads=True)
        bad = 0
        for it in range(300):
            e.rng.fill_(123)
            g.replay()
            if it % 10 == 0 or it > 280:
                y = e._buf("enc.norm.y", 8 * 64, e.dims.hidden).clone()
                if first is None:
                    first = y
                bad += int(not torch.equal(y, first))
        torch.cuda.synchronize()
        assert e.encoder_stack_error() == 0
        assert bad == 0, f"placement {placement}: {bad} replays differed"
        assert torch.isfinite(first).all()


def test_fused_encoder_train_steps_track_the_unfused_engine(mods):
    """A few optimizer steps with the fused encoder against the same steps without it (same seeds, dropout on)."""
    _, _, synthetic = mods
    batch = {k: v.cuda() for k, v in synthetic.synthetic_batch(8, 256, 64, seed=13).items()}
    losses = {}
    for fused in (False, True):
        e = _engine(mods)
        e.train_dropout = True
        e.enc_fused = fused
        ls = []
        for _ in range(6):
            ls.append(e.train_step_graphed(batch).clone())
        torch.cuda.synchronize()
        losses[fused] = torch.stack(ls).cpu()
        if fused:
            assert e.encoder_stack_error() == 0
            assert e.opt_stats()["skipped"] == 0
    assert torch.isfinite(losses[True]).all()
    assert torch.allclose(losses[True][:, 0], losses[False][:, 0], rtol=3e-2), (losses[True][:, 0], losses[False][:, 0])


# ---- bit identity with the commit the digests were recorded at (tools/record_encstack_golden.py) ----------------------------------
# The comparison above allows 6e-3 per layer (the two paths sum their GEMMs in different orders), so it cannot see a drift in the
# code the fused launch shares with the library (sub-layer tail, probability dropout, group barrier).  These cases pin the bits of
# everything the fused forward leaves behind, at the smallest shapes that reach every arm of that code:
#   default dims, 3 x 50 ragged, dropout : enc_stack_fwd_kernel<512,1536>, attn_head<2>, padded keys, both tails with every mask live, no second item
#   default dims, 2 x 97, dropout on/off : attn_head<4>; p = 0: thresholds 0, no seed read
#   smallest dims the launch accepts, 9 x 33 ragged, dropout : enc_stack_fwd_kernel<0,0>, a group walking a second item (b + 8)
# The last layer's FFN tail writes enc.norm.y in fp32 (the next_y arm without bf16) in every case.  DropPath is live in the layers
# past the first; the recorder picks a seed at which one tail drops a sample and keeps another (row / S indexing).
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encstack_parent_digests.json")
SMALL = dict(hidden=128, heads=2, enc_layers=2, dec_layers=1, enc_ff=128, dec_ff=128, var_filter=32, var_bins=16)
DIGEST_CASES = {      # id: (ModelDims arguments, B, T, P, ragged, dropout)
    "default-3x50-ragged-drop": ({}, 3, 96, 50, True, True),
    "default-2x97-drop": ({}, 2, 160, 97, False, True),
    "default-2x97-nodrop": ({}, 2, 160, 97, False, False),
    "small-9x33-ragged-drop": (SMALL, 9, 64, 33, True, True),
}


def _digest(t):
    t = t.detach().cpu().contiguous()
    raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")}


def fused_encoder_tensors(mods, engines, case, placement, seed):
    """Everything the fused encoder forward of DIGEST_CASES[case] leaves behind (engines: a dict that keeps one engine per dims)."""
    _, spec, synthetic = mods
    kw, B, T, P, ragged, dropout = DIGEST_CASES[case]
    key = tuple(sorted(kw.items()))
    if key not in engines:
        engines[key] = _engine(mods, spec.ModelDims(**kw))
        engines[key].enc_fused_max_batch = 64
    e = engines[key]
    e.train_dropout = dropout
    assert e._encoder_stack_ok(B, P), "the shape must be served by the fused launch"
    batch = {k: v.cuda() for k, v in synthetic.synthetic_batch(B, T, P, mel=e.dims.mel, seed=5, ragged=ragged).items()}
    got, _ = _forward(e, batch, fused=True, placement=placement, seed=seed)
    assert e.encoder_stack_error() == 0, "a group barrier of the fused encoder timed out"
    return got


def droppath_is_exercised(got, layers, B):
    """True when some sub-layer tail past the first layer dropped a whole sample (stream out == stream in) and kept another."""
    for i in range(1, layers):
        for x_in, x_out in ((got[f"enc{i - 1}.xo"], got[f"enc{i}.xm"]), (got[f"enc{i}.xm"], got[f"enc{i}.xo"])):
            dropped = [torch.equal(a, b) for a, b in zip(x_in.view(B, -1), x_out.view(B, -1))]
            if any(dropped) and not all(dropped):
                return True
    return False


@pytest.fixture(scope="module")
def digest_engines():
    return {}


@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("case", list(DIGEST_CASES))
def test_fused_encoder_bits_match_the_recorded_parent(mods, digest_engines, case, placement):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][case]
    got = fused_encoder_tensors(mods, digest_engines, case, placement, want["seed"])
    have = {k: _digest(v) for k, v in got.items()}
    assert sorted(have) == sorted(want["tensors"])
    differ = [k for k in have if have[k] != want["tensors"][k]]
    assert not differ, f"{case}, placement {placement}: {len(differ)} of {len(have)} tensors differ from the recorded bits: {differ[:8]}"


def test_unsupported_shapes_fall_back(mods):
    e = _engine(mods)
    assert not e._encoder_stack_ok(4, 129)          # longer than a group carries
    e.enc_fused = False
    assert not e._encoder_stack_ok(8, 64)
