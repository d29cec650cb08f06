"""GPU suite, kernel level: the sub-layer tail and dropout kernels of kk_dropout.hip with EXACT masks, against float64, called through
the C ABI (kokoro_ruslan_amd.lib.call).

The masks are pure functions of (seed, call site, element index); tests/dropout_masks.py restates them on the host, so a test knows
every mask bit of a launch.

Part A — the masks are the replica's: kk_dropout_fwd of ones IS the mask (torch.equal against the replica, 1/(1-p) being the fp32
division of the kernel), the DropPath sample boundary, the second trip of the grid-stride loop, the periodic residual; kk_glu_fwd /
kk_embed_fwd (indexed row * width + col) and kk_specaug against the same replica.
Part B — kk_sublayer_out_fwd against float64 with the explicit mask, at every NV arm, dead lanes, and the plain-store path.
Part C — kk_sublayer_in_bwd against float64 closed forms with the explicit mask, at every (NV, waves, RIF) arm.

Bound (tests/fp64_bounds.py, the rule of test_norm_kernels_gpu.py): kernel error <= 4 E_ref + 2^-22 (+ 2^-8 for a bf16 output), all
normalised by max|fp64|, E_ref being the error of an fp32 PyTorch restatement on the same inputs with the same mask.  Every check
prints E_ref, the kernel's error and their ratio (pytest -s); docs/LAB_NOTES.md "Tail kernels vs fp64" holds what was measured.
Every output lives in a guarded buffer (sentinel rows around it, NaN inside before the launch).

Part B2 — the bits of kk_sublayer_out_fwd and kk_linear_tail_fwd are the ones recorded at the parent of csrc/kk_tail.h.

kk_linear_tail_fwd needs no fp64 case here: test_kernels_gpu.py::test_linear_tail_fwd_matches_two_launches ties it bit for bit to
kk_gemm + kk_sublayer_out_fwd at eight shapes of H = 512, so anchoring kk_sublayer_out_fwd at H = 512 (below) anchors it too."""
import functools
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_masks as DM  # noqa: E402
import fp64_bounds as FB  # noqa: E402
from fp64_bounds import BF16_ROUND, FLT_EPS, NAN, Guarded, gvec  # noqa: E402

pytestmark = pytest.mark.gpu

bounded = functools.partial(FB.bounded, tag="tail-fp64")
SEED, SITE1, SITE2, SITE_DP = 77, 40, 41, 42
ULP = 2.0 ** -23                                   # one unit in the last place of an fp32 number is at most 2^-23 of its value
MASKS = [(0.2, 0.1, 0.25), (0.0, 0.2, 0.0), (0.2, 0.0, 0.0), (0.0, 0.0, 0.0)]
# (rows, H, S): NV1, 16 live lanes, rows % 4 = 1 | NV2, one live lane in slab 2 | the model's width | NV4 at nv = 3 | NV8 begins |
# NV8 full, DropPath per row | plain stores (rows > 16384), 2 live lanes
FWD_SHAPES = [(37, 64, 5), (21, 260, 4), (19, 512, 4), (13, 768, 3), (9, 1028, 2), (6, 2048, 1), (16389, 8, 7)]
# ... | NV1, RIF 1, 256 workgroups, three trips | RIF 2 with no second row | NV2, RIF 1 (no other shape takes that arm)
BWD_SHAPES = FWD_SHAPES + [(4129, 64, 40), (6, 64, 2), (4100, 260, 41)]
WT_MAX_ROWS = 16384                                # kk_common.h KK_WT_MAX_ROWS: above it the tails store plainly


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def dev(t):
    return t.cuda().contiguous()


def _r16(t):
    return t.bfloat16().float()


def _seed():
    return torch.tensor([SEED], dtype=torch.int32, device="cuda")


def _nv(H):
    nv = -(-H // 256)
    return 1 if nv <= 1 else (2 if nv <= 2 else (4 if nv <= 4 else 8))


@functools.lru_cache(maxsize=None)
def _masks(rows, H, S, p1, p2, dp):
    """(float64 multiplier, the same from the kernels' fp32 1/(1-p) factors, keep_dp per row) as CPU tensors, after asserting from
    the replica that the data can show a fault: with DropPath at least one sample kept and one dropped; with element dropout both
    kept and dropped elements in every row (a row of fewer than 64 elements cannot promise that — 0.8^8 of the 8-wide rows keep
    everything — so there it is every run of 64 / H whole rows)."""
    args = (SEED, rows, H, S, SITE1, p1, SITE2, p2, SITE_DP, dp)
    k1, k2, kd = DM.tail_keeps(*args)
    if dp > 0 and rows > S:
        assert kd.any() and not kd.all(), f"{rows}x{H} S={S}: DropPath keeps or drops every sample (the data is wrong, not the kernel)"
    if p1 > 0 or p2 > 0:
        k = k1 & k2
        if H < 64:
            g = 64 // H
            k = k[:rows // g * g].reshape(rows // g, g * H)
        assert bool((k.any(1) & (~k).any(1)).all()), f"{rows}x{H}: a row without a kept or without a dropped element"
    return torch.from_numpy(DM.tail_mask(*args)), torch.from_numpy(DM.tail_mask(*args, fp32_factors=True)), torch.from_numpy(kd)


def _mask32(m32f):
    """The fp32 restatement's multiplier: the product of the fp32 factors, rounded to fp32 (exact when only one rate is set)."""
    return m32f.float()


def _clean(*bufs):
    for b in bufs:
        assert b.intact(), "a guard row / column was written"
        assert not bool(torch.isnan(b.t.float()).any()), "a NaN is left: an element was not written"


# ------------------------------------------------------------------ part A: the masks are exactly the replica's
# (37, 64, 5): the last sample is partial | (2049, 2048, 64): rows * H / 4 > 4096 * 256, a second trip of the grid-stride loop
DROP_SHAPES = [(37, 64, 5), (2049, 2048, 64)]


@pytest.mark.parametrize("which", ["p1", "p2", "dp", "all"])
@pytest.mark.parametrize("rows,H,S", DROP_SHAPES)
def test_dropout_fwd_of_ones_is_the_replica_mask(kk, rows, H, S, which):
    p1, p2, dp = {"p1": (0.2, 0.0, 0.0), "p2": (0.0, 0.1, 0.0), "dp": (0.0, 0.0, 0.25), "all": (0.2, 0.1, 0.25)}[which]
    if rows == 2049:
        assert rows * H // 4 > 4096 * 256, "more float4s than the capped grid has threads: a second trip of the loop"
    _, m32f, kd = _masks(rows, H, S, p1, p2, dp)
    out = Guarded(rows, H)
    kk.call("kk_dropout_fwd", torch.ones(rows, H, device="cuda"), None, 0, out.t, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp)
    torch.cuda.synchronize()
    _clean(out)
    got = out.t.cpu().double()
    assert torch.equal(got != 0, m32f != 0), f"{which} {rows}x{H}: the kept set is not the replica's " \
                                             f"({int(((got != 0) != (m32f != 0)).sum())} elements differ)"
    if which == "all":
        err = float(((got - m32f).abs() / m32f.clamp(min=1.0)).max())
        print(f"[tail-fp64] dropout fwd of ones {rows}x{H} all three: max relative error {err:.3e} (one ulp = {ULP:.3e})")
        assert err <= ULP, "rs * m1 * m2 is two fp32 roundings of the three fp32 factors: within one ulp of their product"
    else:
        assert torch.equal(got, m32f), f"{which} {rows}x{H}: kept elements are 1.f / (1.f - p), dropped are 0"
    if dp > 0:
        assert bool((got[~kd] == 0).all()) and bool((got[kd] != 0).any(1).all()), "DropPath drops whole samples of S rows"


@pytest.mark.parametrize("rows,H,S", DROP_SHAPES)
def test_dropout_bwd_regenerates_the_replica_mask(kk, rows, H, S):
    """dx = dy * mask elementwise (rs * m1 * m2, then * dy: three fp32 roundings, 3 * 2^-24 <= 2^-22 of the value); the bf16 output is
    the rounded fp32 output."""
    p1, p2, dp = MASKS[0]
    m64, _, _ = _masks(rows, H, S, p1, p2, dp)
    g = torch.Generator().manual_seed(rows + H)
    dy = torch.randn(rows, H, generator=g)
    dx, dx16 = Guarded(rows, H), Guarded(rows, H, dtype=torch.bfloat16)
    dyd = dev(dy)
    kk.call("kk_dropout_bwd", dyd, dx.t, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp, 0)
    kk.call("kk_dropout_bwd", dyd, dx16.t, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp, 1)
    torch.cuda.synchronize()
    _clean(dx, dx16)
    ref, got = dy.double() * m64, dx.t.cpu().double()
    assert torch.equal(got != 0, ref != 0), "the backward's kept set is not the replica's"
    err = float(((got - ref).abs() / ref.abs().clamp(min=1e-30)).max())
    print(f"[tail-fp64] dropout bwd {rows}x{H}: max relative error {err:.3e} (allowed 2^-22 = {FB.FLOOR:.3e})")
    assert err <= FB.FLOOR
    assert torch.equal(dx16.t, dx.t.bfloat16()), "bf16 output = rounded fp32 output"


def test_dropout_fwd_periodic_residual_exact(kk):
    """res_mod = S at p = 0: out = x + res[row % S], one fp32 addition."""
    rows, H, S = 37, 64, 5
    g = torch.Generator().manual_seed(1)
    x, pe = torch.randn(rows, H, generator=g), torch.randn(S, H, generator=g)
    out = Guarded(rows, H)
    kk.call("kk_dropout_fwd", dev(x), dev(pe), S, out.t, rows, H, S, _seed(), SITE1, 0.0, SITE2, 0.0, SITE_DP, 0.0)
    torch.cuda.synchronize()
    _clean(out)
    assert torch.equal(out.t.cpu(), x + pe[torch.arange(rows) % S])
    _, m32f, _ = _masks(rows, H, S, 0.2, 0.0, 0.0)                      # and with a mask: fl(x * k) + pe, dropped -> pe exactly
    kk.call("kk_dropout_fwd", dev(x), dev(pe), S, out.t, rows, H, S, _seed(), SITE1, 0.2, SITE2, 0.0, SITE_DP, 0.0)
    torch.cuda.synchronize()
    _clean(out)
    want = (x * _mask32(m32f)).double() + pe[torch.arange(rows) % S].double()
    got = out.t.cpu()
    assert torch.equal(got[m32f == 0], pe[torch.arange(rows) % S][m32f == 0]), "a dropped element is the residual, bit for bit"
    assert float((got.double() - want).abs().max()) <= ULP * float(want.abs().max()), "x * k + res: a product and a sum (or one fma)"


def _one_ulp_of(got, base, mask32f, what):
    """got == base * mask within one ulp (base is the p = 0 output of the same kernel, the mask one fp32 factor)."""
    ref = base.cpu().double() * mask32f
    got = got.cpu().double()
    assert torch.equal(got[mask32f == 0], torch.zeros_like(got[mask32f == 0])), f"{what}: a dropped element is not zero"
    assert bool(((got != 0) | (ref == 0)).all()), f"{what}: a kept element is zero"
    err = float(((got - ref).abs() / ref.abs().clamp(min=1e-30)).max())
    print(f"[tail-fp64] {what}: max relative error against p = 0 output x replica mask {err:.3e} (one ulp = {ULP:.3e})")
    assert err <= ULP, what


def test_glu_and_embed_masks_are_indexed_row_times_width_plus_col(kk):
    g = torch.Generator().manual_seed(2)
    rows, Fd, p, site = 37, 20, 0.2, 3
    h = torch.randn(rows, 2 * Fd, generator=g) + 1.0
    g0, g1 = Guarded(rows, Fd), Guarded(rows, Fd)
    kk.call("kk_glu_fwd", dev(h), g0.t, rows, Fd, None, 0, 0.0, 0)
    kk.call("kk_glu_fwd", dev(h), g1.t, rows, Fd, _seed(), site, p, 0)
    torch.cuda.synchronize()
    _clean(g0, g1)
    keep = DM.keep(SEED, site, np.arange(rows * Fd).reshape(rows, Fd), p)
    assert keep.any(1).all() and (~keep).any(), "the data is wrong, not the kernel"
    assert float(g0.t.abs().min()) > 0
    _one_ulp_of(g1.t, g0.t, torch.from_numpy(keep * float(DM.inv_keep32(p))), f"glu fwd {rows}x{Fd}")
    B, P, H, V, pe_p, site = 3, 7, 12, 11, 0.15, 1
    ids, stress = torch.randint(1, V, (B, P), generator=g), torch.randint(0, 3, (B, P), generator=g)
    emb, semb, pe = torch.randn(V, H, generator=g), torch.randn(3, H, generator=g), torch.randn(P, H, generator=g)
    args = (dev(ids), dev(stress), dev(emb), dev(semb), dev(pe))
    o0, o1 = Guarded(B * P, H), Guarded(B * P, H)
    kk.call("kk_embed_fwd", *args, o0.t, B, P, H, 8.0, None, 0, 0.0)
    kk.call("kk_embed_fwd", *args, o1.t, B, P, H, 8.0, _seed(), site, pe_p)
    torch.cuda.synchronize()
    _clean(o0, o1)
    keep = DM.keep(SEED, site, np.arange(B * P * H).reshape(B * P, H), pe_p)
    assert keep.any() and (~keep).any() and float(o0.t.abs().min()) > 0, "the data is wrong, not the kernel"
    _one_ulp_of(o1.t, o0.t, torch.from_numpy(keep * float(DM.inv_keep32(pe_p))), f"embed fwd {B}x{P}x{H}")


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("T", [9, 3])
def test_specaug_zeroes_exactly_the_replica_set(kk, T, bf16):
    """T = 9: time limit min(20, 9 // 4) = 2.  T = 3: time limit max(1, 0) = 1, every length 0, no time mask."""
    B, H, site, tmax, fmax, nt, nf = 3, 12, 20, 20, 5, 2, 2
    zero = torch.from_numpy(DM.specaug_zero(SEED, site, B, T, H, tmax, fmax, nt, nf))
    if T == 9:
        assert bool(zero.all(2).any()) and bool(zero.all(1).any()) and not bool(zero.all()), "the data is wrong, not the kernel"
    else:
        assert not bool(zero.all(2).any()) and bool(zero.any())
    g = torch.Generator().manual_seed(T)
    x = _r16(torch.rand(B * T, H, generator=g) + 1.0)
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = Guarded(B * T, H, dtype=dt, fill=x.cuda().to(dt))
    kk.call("kk_specaug", buf.t, B, T, H, _seed(), site, tmax, fmax, nt, nf, bf16)
    torch.cuda.synchronize()
    _clean(buf)
    assert torch.equal(buf.t.cpu().float(), torch.where(zero.view(B * T, H), torch.zeros_like(x), x))


# ------------------------------------------------------------------ part B: kk_sublayer_out_fwd against float64
# (gain, LayerNorm, y bf16, n bf16, mask set): every value of every axis meets every shape, so every NV arm
FWD_CONFIGS = [(1, 1, 1, 1, 0), (0, 1, 0, 0, 1), (1, 0, 0, 0, 2), (0, 1, 1, 0, 3)]


def _tail_fwd_ref(y, gain, res, mask, gamma, beta, dtype):
    y, res, mask = y.to(dtype), res.to(dtype), mask.to(dtype)
    out = {}
    z = y
    if gain is not None:
        out["rstd_f"] = 1.0 / torch.sqrt((y * y).mean(1) + FLT_EPS)
        z = y * out["rstd_f"][:, None] * gain.to(dtype)
    x = res + z * mask
    out["x_out"] = x
    if gamma is not None:
        mean = x.mean(1)
        rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
        out.update(mean=mean, rstd=rstd, n=(x - mean[:, None]) * rstd[:, None] * gamma.to(dtype) + beta.to(dtype))
    return out


@pytest.mark.parametrize("gain_on,ln,y_bf16,n_bf16,mi", FWD_CONFIGS)
@pytest.mark.parametrize("rows,H,S", FWD_SHAPES)
def test_sublayer_out_fwd_fp64(kk, rows, H, S, gain_on, ln, y_bf16, n_bf16, mi):
    p1, p2, dp = MASKS[mi]
    m64, m32f, kd = _masks(rows, H, S, p1, p2, dp)
    g = torch.Generator().manual_seed(rows * 3 + H + mi)
    y = torch.randn(rows, H, generator=g) * 1.5 + 0.25
    if y_bf16:
        y = _r16(y)                                                      # a bf16 y is exact input
    res = torch.randn(rows, H, generator=g) * 2 + 0.5                    # a mean of the order of the spread, as the stream has
    gain = 1 + 0.25 * torch.randn(H, generator=g) if gain_on else None
    gamma, beta = (1 + 0.25 * torch.randn(H, generator=g), torch.randn(H, generator=g)) if ln else (None, None)
    r64 = _tail_fwd_ref(y, gain, res, m64, gamma, beta, torch.float64)
    r32 = _tail_fwd_ref(y, gain, res, _mask32(m32f), gamma, beta, torch.float32)
    yd = dev(y).bfloat16() if y_bf16 else dev(y)
    x_out, rstd_f = Guarded(rows, H), gvec(rows, NAN)
    n = Guarded(rows, H, dtype=torch.bfloat16 if n_bf16 else torch.float32)
    mean, rstd = gvec(rows, NAN), gvec(rows, NAN)
    kk.call("kk_sublayer_out_fwd", yd, y_bf16, dev(gain) if gain_on else None, rstd_f.t if gain_on else None, dev(res), x_out.t,
            dev(gamma) if ln else None, dev(beta) if ln else None, n.t if ln else None, n_bf16 if ln else 0, mean.t if ln else None,
            rstd.t if ln else None, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp)
    arm = kk.last_kernel()
    torch.cuda.synchronize()
    want_arm = f"sublayer_out_fwd<{2 if y_bf16 else 4},{2 if (ln and n_bf16) else 4},{_nv(H)}>"
    assert arm == want_arm, (arm, want_arm)
    assert (rows > WT_MAX_ROWS) == (rows == 16389), "only the 16389-row shape takes the plain stores"
    tag = f"out_fwd {rows}x{H} S={S} NV{_nv(H)} gain={gain_on} ln={ln} y_bf16={y_bf16} n_bf16={n_bf16} p={p1}/{p2}/{dp}"
    _clean(x_out)
    bounded(f"{tag} x_out", x_out.t, r32["x_out"], r64["x_out"])
    for b, used in ((rstd_f, gain_on), (n, ln), (mean, ln), (rstd, ln)):
        if used:
            _clean(b)
        else:
            assert b.intact() and bool(torch.isnan(b.t.float()).all()), f"{tag}: an output that was not asked for was written"
    if gain_on:
        bounded(f"{tag} rstd_f", rstd_f.t[0], r32["rstd_f"], r64["rstd_f"])
    if ln:
        bounded(f"{tag} mean", mean.t[0], r32["mean"], r64["mean"])
        bounded(f"{tag} rstd", rstd.t[0], r32["rstd"], r64["rstd"])
        bounded(f"{tag} n", n.t, r32["n"], r64["n"], BF16_ROUND if n_bf16 else 0.0)
    if dp > 0:
        assert torch.equal(x_out.t.cpu()[~kd], res[~kd]), f"{tag}: x_out of a dropped sample is the residual, bit for bit"
    if p1 > 0 or p2 > 0:
        drop = m64 == 0
        assert torch.equal(x_out.t.cpu()[drop], res[drop]), f"{tag}: x_out of a dropped element is the residual, bit for bit"


# ------------------------------------------------------------------ part B2: the tail forward's bits are the recorded parent's
# The forward tail is written three times (sublayer_out_row of csrc/kk_tail.h, the fused Linear's epilogue, the encoder stack's tail_row)
# and the other tests only compare the copies with each other.  tests/golden/tail_parent_digests.json ties the first two to their own
# past: the SHA-256 of every output of the launches below as the tree before kk_tail.h computed them (tools/record_tail_golden.py, which
# calls tail_forward_digests too).
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_parent_digests.json")
DIGEST_MASKS = [MASKS[0], (0.0, 0.0, 0.0)]
# kk_linear_tail_fwd at H = 512: (rows, S, K, LayerNorm).  77 rows: the last workgroup holds 13, wave 3 one live row, waves 4 to 7 none;
# K = 64 a single k-tile, 576 a short last chunk
LT_SHAPES = [(77, 5, 64, 1), (77, 5, 576, 1), (45, 7, 512, 0)]
LT_KEEPS = {(77, 5): "1101110010111101", (45, 7): "1101110"}     # DropPath per sample, from the host replica


def _digest(t):
    t = t.detach().cpu().contiguous()
    raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")}


def _sublayer_out_digests(kk, out):
    for (rows, H, S), (p1, p2, dp) in itertools.product(FWD_SHAPES, DIGEST_MASKS):
        _masks(rows, H, S, p1, p2, dp)                                   # asserts that DropPath keeps one sample and drops another
        g = torch.Generator().manual_seed(rows * 7 + H)
        y = torch.randn(rows, H, generator=g) * 1.5 + 0.25
        res = dev(torch.randn(rows, H, generator=g) * 2 + 0.5)
        gain, gamma = dev(1 + 0.25 * torch.randn(H, generator=g)), dev(1 + 0.25 * torch.randn(H, generator=g))
        beta = dev(torch.randn(H, generator=g))
        for y_bf16, n_bf16, gain_on, ln in itertools.product((0, 1), repeat=4):
            yd = dev(y).bfloat16() if y_bf16 else dev(y)
            x_out, rstd_f = Guarded(rows, H), gvec(rows, NAN)
            n = Guarded(rows, H, dtype=torch.bfloat16 if n_bf16 else torch.float32)
            mean, rstd = gvec(rows, NAN), gvec(rows, NAN)
            kk.call("kk_sublayer_out_fwd", yd, y_bf16, gain if gain_on else None, rstd_f.t if gain_on else None, res, x_out.t,
                    gamma if ln else None, beta if ln else None, n.t if ln else None, n_bf16 if ln else 0, mean.t if ln else None,
                    rstd.t if ln else None, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp)
            torch.cuda.synchronize()
            got = {"x_out": x_out}
            if gain_on:
                got["rstd_f"] = rstd_f
            if ln:
                got.update(n=n, mean=mean, rstd=rstd)
            _clean(*got.values())
            out[f"out_fwd {rows}x{H} S={S} y_bf16={y_bf16} n_bf16={n_bf16} gain={gain_on} ln={ln} p={p1}/{p2}/{dp}"] = \
                {k: _digest(b.t) for k, b in got.items()}


def _linear_tail_digests(kk, out):
    H = 512
    for rows, S, K, ln in LT_SHAPES:
        g = torch.Generator().manual_seed(rows + K)
        x = dev(torch.randn(rows, K, generator=g)).bfloat16()
        W = dev(torch.randn(H, K, generator=g) / K ** 0.5).bfloat16()
        bias, res = dev(0.1 * torch.randn(H, generator=g)), dev(torch.randn(rows, H, generator=g) * 2 + 0.5)
        gain, gamma = dev(1 + 0.25 * torch.randn(H, generator=g)), dev(1 + 0.25 * torch.randn(H, generator=g))
        beta = dev(torch.randn(H, generator=g))
        assert kk.load().kk_linear_tail_supported(rows, H, K) == 1
        for ffn, n_bf16 in itertools.product((1, 0), (1, 0) if ln else (0,)):
            p1, p2, dp = (0.2, 0.1, 0.25) if ffn else (0.2, 0.0, 0.25)
            k1, k2, kd = DM.tail_keeps(SEED, rows, H, S, SITE1, p1, SITE2, p2, SITE_DP, dp)
            assert "".join(str(int(v)) for v in kd[::S]) == LT_KEEPS[rows, S], "DropPath per sample is not what the case was chosen for"
            if rows == 77:
                assert kd[8] and kd[9] and not kd[10] and not kd[11], "rows 8 to 11, one wave's four, span a kept and a dropped sample"
            k = k1 & k2
            assert bool((k.any(1) & (~k).any(1)).all()), "a row without a kept or without a dropped element"
            y_out = Guarded(rows, H, dtype=torch.bfloat16)
            x_out, rstd_f = Guarded(rows, H), gvec(rows, NAN)
            n = Guarded(rows, H, dtype=torch.bfloat16 if n_bf16 else torch.float32)
            mean, rstd = gvec(rows, NAN), gvec(rows, NAN)
            # FFN form: y rounded to bf16 and stored for the backward, RMSNorm gain; attention form: fp32 y, not stored
            kk.call("kk_linear_tail_fwd", x, K, W, bias, K, y_out.t if ffn else None, ffn, gain if ffn else None, rstd_f.t if ffn else None,
                    res, x_out.t, gamma if ln else None, beta if ln else None, n.t if ln else None, n_bf16, mean.t if ln else None,
                    rstd.t if ln else None, rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp)
            torch.cuda.synchronize()
            assert kk.last_kernel() == "linear_tail_fwd"
            got = {"x_out": x_out}
            if ffn:
                got.update(y_out=y_out, rstd_f=rstd_f)
            if ln:
                got.update(n=n, mean=mean, rstd=rstd)
            _clean(*got.values())
            for b in (y_out, rstd_f, n, mean, rstd):
                if not any(b is u for u in got.values()):
                    assert b.intact() and bool(torch.isnan(b.t.float()).all()), "an output that was not asked for was written"
            out[f"linear_tail {rows}x{H} S={S} K={K} ffn={ffn} ln={ln} n_bf16={n_bf16}"] = {k: _digest(b.t) for k, b in got.items()}


def tail_forward_digests(kk):
    """{case: {output: digest}} of every forward tail launch whose bits are pinned (the recorder and the test below share this)."""
    out = {}
    _sublayer_out_digests(kk, out)
    _linear_tail_digests(kk, out)
    return out


def test_tail_forward_bits_match_the_recorded_parent(kk):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    have = tail_forward_digests(kk)
    assert sorted(have) == sorted(want)
    differ = [f"{c}: {k}" for c in have for k in sorted(set(have[c]) | set(want[c])) if have[c].get(k) != want[c].get(k)]
    assert not differ, f"{len(differ)} outputs of {len(have)} launches differ from the recorded bits: {differ[:8]}"


# ------------------------------------------------------------------ part C: kk_sublayer_in_bwd against float64
# (accumulate, dn bf16, y / dy bf16, gain, mask set)
BWD_CONFIGS = [(1, 1, 1, 1, 0), (0, 0, 0, 0, 1), (1, 0, 1, 0, 2), (0, 1, 0, 1, 3)]


def _tail_bwd_ref(dn, x_out, gamma, mean, rstd, dres0, mask, y, gain, rstd_f, dtype):
    c = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    dn, x_out, gamma, mean, rstd, dres0, mask, y, gain, rstd_f = map(c, (dn, x_out, gamma, mean, rstd, dres0, mask, y, gain, rstd_f))
    dx, tg = FB.ln_bwd_formula(dn, x_out, gamma, mean, rstd)
    gres = dx if dres0 is None else dres0 + dx
    out = dict(dres=gres, dgamma=tg.sum(0), dbeta=dn.sum(0))
    dz = gres * mask
    if gain is not None:
        dy, tn = FB.rms_bwd_formula(dz, y, gain, rstd_f)
        out["dgain"] = tn.sum(0)
    else:
        dy = dz
    out.update(dy=dy, dbias=dy.sum(0))
    return out


def _bwd_arm(kk, rows, H):
    """(workgroups, waves per workgroup, rows in flight) as launch_subin chooses them."""
    nb = kk.load().kk_sublayer_in_bwd_blocks(rows)
    assert nb == max(1, min(256, -(-rows // 16)))
    nv = _nv(H)
    waves = 8 if nv <= 2 else (4 if nv == 4 else 2)
    rif = 2 if (nv <= 2 and rows <= 2 * nb * 8) else 1
    return nb, waves, rif


@pytest.mark.parametrize("acc,dn_bf16,y_bf16,gain_on,mi", BWD_CONFIGS)
@pytest.mark.parametrize("rows,H,S", BWD_SHAPES)
def test_sublayer_in_bwd_fp64(kk, rows, H, S, acc, dn_bf16, y_bf16, gain_on, mi):
    p1, p2, dp = MASKS[mi]
    m64, m32f, kd = _masks(rows, H, S, p1, p2, dp)
    nb, waves, rif = _bwd_arm(kk, rows, H)
    if (rows, H) == (37, 64):
        assert (nb, waves, rif) == (3, 8, 2) and [w for w in range(24) if w + 24 >= rows] == list(range(13, 24)), \
            "waves 13 to 23 of the 24 have a dead second row"
    if (rows, H) == (6, 64):
        assert (nb, waves, rif) == (1, 8, 2), "RIF 2 with no second row at all"
    if (rows, H) == (4129, 64):
        assert (nb, waves, rif) == (256, 8, 1) and -(-rows // (nb * waves)) == 3, "RIF 1, 256 workgroups, three trips"
    if (rows, H) == (4100, 260):
        assert (nb, waves, rif) == (256, 8, 1) and _nv(H) == 2
    g = torch.Generator().manual_seed(rows * 5 + H + mi)
    x_out = torch.randn(rows, H, generator=g) * 2 + 0.5
    dn, y, dres0 = torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g) * 1.5 + 0.25, torch.randn(rows, H, generator=g)
    if dn_bf16:
        dn = _r16(dn)
    if y_bf16:
        y = _r16(y)
    gamma = 1 + 0.25 * torch.randn(H, generator=g)
    gain = 1 + 0.25 * torch.randn(H, generator=g) if gain_on else None
    # the statistics a forward would have saved: the fp32 roundings of the float64 statistics of these x_out / y
    x64, y64 = x_out.double(), y.double()
    mean = x64.mean(1).float()
    rstd = (1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-5)).float()
    rstd_f = (1.0 / torch.sqrt((y64 * y64).mean(1) + FLT_EPS)).float() if gain_on else None
    common = (dn, x_out, gamma, mean, rstd, dres0 if acc else None)
    r64 = _tail_bwd_ref(*common, m64, y if gain_on else None, gain, rstd_f, torch.float64)
    r32 = _tail_bwd_ref(*common, _mask32(m32f), y if gain_on else None, gain, rstd_f, torch.float32)
    dnd = dev(dn).bfloat16() if dn_bf16 else dev(dn)
    ydt = torch.bfloat16 if y_bf16 else torch.float32
    dres = Guarded(rows, H, fill=dres0.cuda() if acc else NAN)
    dy, part = Guarded(rows, H, dtype=ydt), Guarded(nb, 4 * H)
    kk.call("kk_sublayer_in_bwd", dnd, dn_bf16, dev(x_out), dev(gamma), dev(mean), dev(rstd), dres.t, acc,
            dev(y).to(ydt) if gain_on else None, dev(gain) if gain_on else None, dev(rstd_f) if gain_on else None, dy.t, y_bf16, part.t,
            rows, H, S, _seed(), SITE1, p1, SITE2, p2, SITE_DP, dp)
    torch.cuda.synchronize()
    tag = f"in_bwd {rows}x{H} S={S} NV{_nv(H)}/{waves}w/RIF{rif} acc={acc} dn_bf16={dn_bf16} y_bf16={y_bf16} gain={gain_on} p={p1}/{p2}/{dp}"
    _clean(dres, dy, part)
    dgam, dbet, dbias, dgain = (gvec(H, 0.0) for _ in range(4))
    table = kk.reduce_table([(part.t, dgam.t, dbet.t, nb, 2 * H, H, 4 * H),
                             (part.t[:, 2 * H:], dbias.t, dgain.t if gain_on else None, nb, 2 * H if gain_on else H, H, 4 * H)], "cuda")
    kk.call("kk_partials_reduce", table, 2, 2 * H)
    torch.cuda.synchronize()
    _clean(dgam, dbet, dbias, dgain, part)
    bounded(f"{tag} dres", dres.t, r32["dres"], r64["dres"])
    bounded(f"{tag} dy", dy.t, r32["dy"], r64["dy"], BF16_ROUND if y_bf16 else 0.0)
    bounded(f"{tag} dgamma", dgam.t[0], r32["dgamma"], r64["dgamma"])
    bounded(f"{tag} dbeta", dbet.t[0], r32["dbeta"], r64["dbeta"])
    bounded(f"{tag} dbias", dbias.t[0], r32["dbias"], r64["dbias"])         # summed before any bf16 rounding of dy
    if gain_on:
        bounded(f"{tag} dgain", dgain.t[0], r32["dgain"], r64["dgain"])
    else:
        assert float(dgain.t.abs().max()) == 0.0
    if dp > 0:
        assert float(dy.t[(~kd).cuda()].float().abs().max()) == 0.0, f"{tag}: dy of a dropped sample is exactly zero"
    if not gain_on and (p1 > 0 or p2 > 0):
        assert float(dy.t[(m64 == 0).cuda()].float().abs().max()) == 0.0, f"{tag}: dy of a dropped element is exactly zero"
