"""GPU suite, kernel level: the normalisation kernels of kk_norm.hip against float64 at every dispatch edge, called through the
C ABI (kokoro_ruslan_amd.lib.call).

Part 1 — exact sums.  The backward kernels take mean / rstd as inputs, so the test chooses them: with dyadic data every product and
every column sum is exactly representable in fp32, whatever the order of the atomics or partial rows is, and dgamma / dbeta / dgain
must EQUAL the float64 sums (the test proves the exactness on the host first).  The shapes are the smallest that reach a second
trip of the grid-stride loop with a ragged R-row group, every template arm (NV 1/2/4/8, R 4/4/2/1) and a partly dead last slab.

Part 2 — accuracy.  The bound is not a fixed number: E_ref = max|fp32 PyTorch restatement - fp64| / max|fp64| on the same inputs,
and the kernel's error, normalised the same way, must be <= 4 E_ref + 2^-22 (4x: another summation tree; 2^-22: the floor where
the restatement happens to be exact); a bf16 output gets one more bf16 rounding, 2^-8.  Every check prints both numbers
(pytest -s); docs/LAB_NOTES.md "Norm kernels vs fp64" holds what was measured."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import kokoro_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_bounds as FB  # noqa: E402
from fp64_bounds import BF16_ROUND, FLT_EPS, NAN, Guarded, gvec  # noqa: E402
from fp64_bounds import ln_bwd_formula as _ln_formula, rms_bwd_formula as _rms_formula  # noqa: E402

pytestmark = pytest.mark.gpu

bounded = functools.partial(FB.bounded, tag="norm-fp64")     # kernel error <= 4 E_ref + 2^-22 (+ extra); prints "[norm-fp64] ..."


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


# ------------------------------------------------------------------ part 1: exact column sums
# (rows, H): second trip with a ragged R-group at NV1/R4 | NV2, dead lanes in the last slab | NV4/R2 at nv = 3 | NV8/R1 begins, 4 live
# columns in slab 5 | NV8/R1 | fewer rows than one workgroup, H < 256 | one wave, exactly one workgroup, one more
EXACT_SHAPES = [(4096 + 5, 64), (4096 + 16 * 3 + 1, 320), (2048 + 3, 768), (2048 + 2, 1028), (1024 + 1, 2048), (7, 80), (1, 512),
                (4, 512), (5, 512)]


def _prove_exact(terms64, start64, what):
    """Every term is an fp32 number, and their fp32 column sums onto `start`, added strictly one row after the other in two random
    row orders, equal the float64 sums bit for bit: then any order of fp32 additions gives these bits."""
    t32 = terms64.float()
    assert torch.equal(t32.double(), terms64), f"{what}: a term is not an fp32 number (the data is wrong, not the kernel)"
    want = start64 + terms64.sum(0)
    assert torch.equal(want.float().double(), want), f"{what}: a column sum is not an fp32 number"
    for seed in (1, 2):
        acc = start64.float().clone()
        for r in torch.randperm(terms64.shape[0], generator=torch.Generator().manual_seed(seed)).tolist():
            acc += t32[r]
        assert torch.equal(acc.double(), want), f"{what}: fp32 sums depend on the order (the data is wrong, not the kernel)"
    return want


@functools.lru_cache(maxsize=None)
def _dyadic(rows, H):
    """x, mean: multiples of 1/4 in [-4, 4]; rstd in {0.5, 1, 2}; dy: multiples of 1/4 in [-2, 2]; gamma in +-{0.5, 1, 2}:
    |dy xhat| <= 32 at resolution 2^-5, so a sum over <= 8192 rows needs at most 24 bits."""
    g = torch.Generator().manual_seed(1000 * H + rows)

    def quarter(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float() / 4

    def pick(vals, *shape):
        return torch.tensor(vals)[torch.randint(0, len(vals), shape, generator=g)]

    d = dict(x=quarter(-16, 16, rows, H), dy=quarter(-8, 8, rows, H), mean=quarter(-16, 16, rows), rstd=pick([0.5, 1.0, 2.0], rows),
             gamma=pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], H), start=quarter(-6, 6, 3, H), dx0=torch.randn(rows, H, generator=g))
    for k in ("x", "dy"):
        assert torch.equal(_r16(d[k]), d[k]), "dyadic values are bf16 numbers"
    return d


@functools.lru_cache(maxsize=None)
def _ln_exact(rows, H):
    d = _dyadic(rows, H)
    a64 = [d[k].double() for k in ("dy", "x", "gamma", "mean", "rstd")]
    dx64, t64 = _ln_formula(*a64)
    dx32, _ = _ln_formula(*[d[k] for k in ("dy", "x", "gamma", "mean", "rstd")])
    dgamma = _prove_exact(t64, d["start"][0].double(), f"dgamma {rows}x{H}")
    dbeta = _prove_exact(a64[0], d["start"][1].double(), f"dbeta {rows}x{H}")
    return dict(d, dx64=dx64, dx32=dx32, dgamma=dgamma, dbeta=dbeta)


@functools.lru_cache(maxsize=None)
def _rms_exact(rows, H):
    d = _dyadic(rows, H)
    dx64, t64 = _rms_formula(*[d[k].double() for k in ("dy", "x", "gamma", "rstd")])
    dx32, _ = _rms_formula(*[d[k] for k in ("dy", "x", "gamma", "rstd")])
    return dict(d, dx64=dx64, dx32=dx32, dgain=_prove_exact(t64, d["start"][2].double(), f"dgain {rows}x{H}"))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dy_bf16", [0, 1])
@pytest.mark.parametrize("rows,H", EXACT_SHAPES)
def test_layernorm_bwd_exact_column_sums(kk, rows, H, dy_bf16, acc):
    """dgamma / dbeta equal the float64 column sums through the atomic exit (onto a non-zero start value) and through partial rows +
    kk_partials_reduce (which leave the gradient vectors alone until the reduce); dx within the bound of part 2; guards untouched;
    with dx_accumulate = 0 nothing of a NaN-filled dx survives."""
    d = _ln_exact(rows, H)
    dy = dev(d["dy"]).bfloat16() if dy_bf16 else dev(d["dy"])
    x, gamma, mean, rstd = dev(d["x"]), dev(d["gamma"]), dev(d["mean"]), dev(d["rstd"])
    nb = kk.load().kk_norm_bwd_blocks(rows, H)
    r = 4 if H <= 512 else (2 if H <= 1024 else 1)
    assert nb == min(256, -(-rows // (4 * r)))
    dx32, dx64 = (d["dx32"] + d["dx0"], d["dx64"] + d["dx0"].double()) if acc else (d["dx32"], d["dx64"])
    dxs = []
    for use_part in (0, 1):
        dx = Guarded(rows, H, fill=d["dx0"].cuda() if acc else NAN)
        dg, db = gvec(H, d["start"][0].cuda()), gvec(H, d["start"][1].cuda())
        part = Guarded(nb, 2 * H)
        kk.call("kk_layernorm_bwd", dy, x, gamma, mean, rstd, dx.t, acc, dg.t, db.t, part.t if use_part else None, rows, H, dy_bf16)
        what = f"ln bwd {rows}x{H} dy_bf16={dy_bf16} acc={acc} {'partials' if use_part else 'atomics'}"
        if use_part:
            assert torch.equal(dg.t[0].cpu(), d["start"][0]) and torch.equal(db.t[0].cpu(), d["start"][1]), \
                f"{what}: with partial rows the launch must not touch the gradient vectors"
            assert bool(torch.isfinite(part.t).all()), f"{what}: a partial row was not written"
            kk.call("kk_partials_reduce", kk.reduce_table([(part.t, dg.t, db.t, nb, 2 * H, H)], "cuda"), 1, 2 * H)
        else:
            assert bool(torch.isnan(part.t).all())
        torch.cuda.synchronize()
        assert dx.intact() and dg.intact() and db.intact() and part.intact(), f"{what}: a guard row / column was written"
        assert torch.equal(dg.t[0].double().cpu(), d["dgamma"]), f"{what}: dgamma is not the exact sum"
        assert torch.equal(db.t[0].double().cpu(), d["dbeta"]), f"{what}: dbeta is not the exact sum"
        bounded(f"{what} dx", dx.t, dx32, dx64)
        dxs.append(dx.t.clone())
    assert torch.equal(dxs[0], dxs[1]), "dx does not depend on the exit of the column sums"


@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("rows,H", EXACT_SHAPES)
def test_rmsnorm_bwd_exact_column_sums(kk, rows, H, x_bf16):
    """dgain equals the float64 column sum through both exits; dx (fp32, or bf16 beside a bf16 x) within the bound of part 2."""
    d = _rms_exact(rows, H)
    x = dev(d["x"]).bfloat16() if x_bf16 else dev(d["x"])
    dy, gain, rstd = dev(d["dy"]), dev(d["gamma"]), dev(d["rstd"])
    nb = kk.load().kk_norm_bwd_blocks(rows, H)
    dxs = []
    for use_part in (0, 1):
        dx = Guarded(rows, H, dtype=torch.bfloat16 if x_bf16 else torch.float32)
        dg, part = gvec(H, d["start"][2].cuda()), Guarded(nb, H)
        kk.call("kk_rmsnorm_bwd", dy, x, gain, rstd, dx.t, dg.t, part.t if use_part else None, rows, H, x_bf16)
        what = f"rms bwd {rows}x{H} x_bf16={x_bf16} {'partials' if use_part else 'atomics'}"
        if use_part:
            assert torch.equal(dg.t[0].cpu(), d["start"][2]), f"{what}: with partial rows the launch must not touch dgain"
            assert bool(torch.isfinite(part.t).all()), f"{what}: a partial row was not written"
            kk.call("kk_partials_reduce", kk.reduce_table([(part.t, dg.t, None, nb, H, H)], "cuda"), 1, H)
        else:
            assert bool(torch.isnan(part.t).all())
        torch.cuda.synchronize()
        assert dx.intact() and dg.intact() and part.intact(), f"{what}: a guard row / column was written"
        assert torch.equal(dg.t[0].double().cpu(), d["dgain"]), f"{what}: dgain is not the exact sum"
        bounded(f"{what} dx", dx.t, d["dx32"], d["dx64"], BF16_ROUND if x_bf16 else 0.0)
        dxs.append(dx.t.clone())
    assert torch.equal(dxs[0], dxs[1]), "dx does not depend on the exit of the column sums"


# ------------------------------------------------------------------ part 2: LayerNorm / RMSNorm on hard inputs
HARD_SHAPES = [(37, 80), (129, 320), (300, 768), (40, 2048)]
KINDS = ["control", "cancel", "constant", "scales"]
CONSTS = [3.0, -2.5, 0.0, 1024.0, 0.375, -96.0]        # few significant bits: H of them sum exactly in any order


def _hard(kind, rows, H, g, zero_rows):
    """control: N(0,1) 2 + 0.5 | cancel: mean 100, std 0.01 | constant: every third row constant (RMSNorm: all zero) | scales: rows of
    magnitude 1e4 and 1e-4 alternate.  Returns (x, indices of the constant rows)."""
    x = torch.randn(rows, H, generator=g) * 2 + 0.5
    const = torch.arange(1, rows, 3)
    if kind == "cancel":
        x = 100 + 0.01 * torch.randn(rows, H, generator=g)
    elif kind == "constant":
        vals = torch.tensor([0.0 if zero_rows else CONSTS[i % len(CONSTS)] for i in range(len(const))])
        x[const] = vals[:, None].expand(-1, H)
    elif kind == "scales":
        x = x * torch.where(torch.arange(rows) % 2 == 0, 1e4, 1e-4)[:, None]
    return x, (const if kind == "constant" else const[:0])


def _ln_ref(x, gamma, beta, dy, dtype):
    xr, gr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xr, (x.shape[1],), gr, br, 1e-5)
    y.backward(dy.to(dtype))
    _, mean, rstd = torch.native_layer_norm(x.to(dtype), (x.shape[1],), gamma.to(dtype), beta.to(dtype), 1e-5)
    return dict(y=y.detach(), mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,H", HARD_SHAPES)
def test_layernorm_fp64(kk, rows, H, kind):
    g = torch.Generator().manual_seed(rows * 7 + H + KINDS.index(kind))
    x, const = _hard(kind, rows, H, g, zero_rows=False)
    gamma, beta = 1 + 0.25 * torch.randn(H, generator=g), torch.randn(H, generator=g)
    dy = _r16(torch.randn(rows, H, generator=g))                  # bf16 numbers: the dy_bf16 launch reads the same values
    r32, r64 = _ln_ref(x, gamma, beta, dy, torch.float32), _ln_ref(x, gamma, beta, dy, torch.float64)
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    tag = f"ln {kind} {rows}x{H}"
    y, y16 = Guarded(rows, H), Guarded(rows, H, dtype=torch.bfloat16)
    mean, rstd, m16, s16 = (gvec(rows, NAN) for _ in range(4))
    kk.call("kk_layernorm_fwd", xd, gd, bd, y.t, mean.t, rstd.t, rows, H, 0)
    kk.call("kk_layernorm_fwd", xd, gd, bd, y16.t, m16.t, s16.t, rows, H, 1)
    torch.cuda.synchronize()
    assert all(b.intact() for b in (y, y16, mean, rstd, m16, s16)), f"{tag}: a guard row / column was written"
    assert torch.equal(m16.t, mean.t) and torch.equal(s16.t, rstd.t) and torch.equal(y16.t, y.t.bfloat16())
    bounded(f"{tag} y", y.t, r32["y"], r64["y"])
    bounded(f"{tag} y bf16", y16.t, r32["y"], r64["y"], BF16_ROUND)
    bounded(f"{tag} mean", mean.t[0], r32["mean"], r64["mean"])
    bounded(f"{tag} rstd", rstd.t[0], r32["rstd"], r64["rstd"])
    if len(const):
        assert torch.equal(y.t[const.cuda()].cpu(), beta.expand(len(const), H)), f"{tag}: y of a constant row is beta, exactly"
        assert torch.equal(y16.t[const.cuda()].cpu(), beta.bfloat16().expand(len(const), H))
        assert torch.equal(mean.t[0][const.cuda()].cpu(), x[const, 0])
        want = 1.0 / torch.sqrt(torch.tensor(1e-5, dtype=torch.float32))
        assert torch.equal(rstd.t[0][const.cuda()].cpu(), want.expand(len(const))), f"{tag}: rstd of a constant row is 1/sqrt(1e-5f)"
    for dy_bf16 in (0, 1):
        dx, dg, db = Guarded(rows, H), gvec(H, 0.0), gvec(H, 0.0)
        kk.call("kk_layernorm_bwd", dev(dy).bfloat16() if dy_bf16 else dev(dy), xd, gd, mean.t, rstd.t, dx.t, 0, dg.t, db.t, None,
                rows, H, dy_bf16)
        torch.cuda.synchronize()
        assert dx.intact() and dg.intact() and db.intact(), f"{tag}: a guard row / column was written"
        bounded(f"{tag} dx dy_bf16={dy_bf16}", dx.t, r32["dx"], r64["dx"])
        bounded(f"{tag} dgamma dy_bf16={dy_bf16}", dg.t[0], r32["dgamma"], r64["dgamma"])
        bounded(f"{tag} dbeta dy_bf16={dy_bf16}", db.t[0], r32["dbeta"], r64["dbeta"])


def _rms(x, w):
    """nn.RMSNorm(eps=None) of an fp32 module: the fp32 restatement is the oracle's; float64 keeps the fp32 module's eps."""
    if x.dtype == torch.float32:
        return O._rms_norm(x, w)
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + FLT_EPS) * w


def _rms_ref(x, gain, res, dy, dtype):
    xr, gr = (t.to(dtype).clone().requires_grad_(True) for t in (x, gain))
    y = res.to(dtype) + _rms(xr, gr)
    y.backward(dy.to(dtype))
    rstd = torch.rsqrt(x.to(dtype).pow(2).mean(-1) + FLT_EPS)
    return dict(y=y.detach(), rstd=rstd, dx=xr.grad, dgain=gr.grad)


@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,H", HARD_SHAPES)
def test_rmsnorm_residual_fp64(kk, rows, H, kind, x_bf16):
    g = torch.Generator().manual_seed(rows * 11 + H + KINDS.index(kind))
    x, zero = _hard(kind, rows, H, g, zero_rows=True)
    if x_bf16:
        x = _r16(x)
    gain, res, dy = 1 + 0.25 * torch.randn(H, generator=g), torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g)
    r32, r64 = _rms_ref(x, gain, res, dy, torch.float32), _rms_ref(x, gain, res, dy, torch.float64)
    xd = dev(x).bfloat16() if x_bf16 else dev(x)
    gd, dyd = dev(gain), dev(dy)
    tag = f"rms {kind} {rows}x{H} x_bf16={x_bf16}"
    y, rstd = Guarded(rows, H), gvec(rows, NAN)
    kk.call("kk_rmsnorm_fwd", xd, gd, dev(res), y.t, rstd.t, rows, H, x_bf16)
    dx, dg = Guarded(rows, H, dtype=torch.bfloat16 if x_bf16 else torch.float32), gvec(H, 0.0)
    kk.call("kk_rmsnorm_bwd", dyd, xd, gd, rstd.t, dx.t, dg.t, None, rows, H, x_bf16)
    torch.cuda.synchronize()
    assert all(b.intact() for b in (y, rstd, dx, dg)), f"{tag}: a guard row / column was written"
    bounded(f"{tag} y", y.t, r32["y"], r64["y"])
    bounded(f"{tag} rstd", rstd.t[0], r32["rstd"], r64["rstd"])
    bounded(f"{tag} dx", dx.t, r32["dx"], r64["dx"], BF16_ROUND if x_bf16 else 0.0)
    bounded(f"{tag} dgain", dg.t[0], r32["dgain"], r64["dgain"])
    if len(zero):
        rs = 1.0 / torch.sqrt(torch.tensor(FLT_EPS, dtype=torch.float32))
        assert torch.equal(y.t[zero.cuda()].cpu(), res[zero]), f"{tag}: y of an all-zero row is the residual, exactly"
        assert torch.equal(rstd.t[0][zero.cuda()].cpu(), rs.expand(len(zero))), f"{tag}: rstd of an all-zero row is 1/sqrt(FLT_EPSILON)"
        want = rs * (dy[zero] * gain)
        assert torch.equal(dx.t[zero.cuda()].cpu(), want.bfloat16() if x_bf16 else want), f"{tag}: dx of an all-zero row is rstd dy gain"


# ------------------------------------------------------------------ per-head RMSNorm(64) + RoPE
def _headnorm_ref(x, gains, dy, cos, sin, heads, S, rope_mask, dtype):
    rows, H = x.shape[0], heads * 64
    pos = torch.arange(rows) % S
    c, s = cos.to(dtype)[pos][:, None, :], sin.to(dtype)[pos][:, None, :]
    xr = x.to(dtype).clone().requires_grad_(True)
    gr = [t.to(dtype).clone().requires_grad_(True) for t in gains]
    outs = []
    for j, gj in enumerate(gr):
        n = _rms(xr[:, j * H:(j + 1) * H].reshape(rows, heads, 64), gj)
        if (rope_mask >> j) & 1:
            n = n * c + O._rotate_half(n) * s
        outs.append(n.reshape(rows, H))
    y = torch.cat(outs, 1)
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), dx=xr.grad, dgain=[t.grad for t in gr])


# (rows, heads, S, parts, rope_mask, bf16).  2048 * 32 + 17 pairs: two full trips of the forward's capped grid (2048 workgroups x 16
# pairs) and of the backward's (512 x 16 x U = 4) and a third of 17 = one 16-lane group more than a row of groups, one pair into a
# U-group.  131 x 3 = 393 pairs = 24 * 16 + 9 = 6 * 64 + 9.  rows % S != 0 and rows > S: positions run to S - 1 and wrap.
HEADNORM_CASES = [(2048 * 32 + 17, 1, 97, 1, 1, 0)] + [(131, 3, 44, 3, m, bf) for bf in (0, 1) for m in (0, 1, 2, 3)] + \
                 [(131, 3, 44, 3, 5, 0), (77, 2, 77, 2, 3, 1)]


@pytest.mark.parametrize("rows,heads,S,parts,rope_mask,bf16", HEADNORM_CASES)
def test_headnorm_rope_fp64(kk, rows, heads, S, parts, rope_mask, bf16):
    g = torch.Generator().manual_seed(rows + 13 * rope_mask + bf16)
    W = parts * heads * 64
    x, dy = torch.randn(rows, W, generator=g) * 2 + 0.5, torch.randn(rows, W, generator=g)
    if bf16:
        x, dy = _r16(x), _r16(dy)
    gains = [torch.rand(64, generator=g) + 0.5 for _ in range(parts)]
    cos, sin = O.rope_tables(S, 64)
    r32 = _headnorm_ref(x, gains, dy, cos, sin, heads, S, rope_mask, torch.float32)
    r64 = _headnorm_ref(x, gains, dy, cos, sin, heads, S, rope_mask, torch.float64)
    dt = torch.bfloat16 if bf16 else torch.float32
    extra = BF16_ROUND if bf16 else 0.0
    xd, dyd, ct, st = dev(x).to(dt), dev(dy).to(dt), dev(cos), dev(sin)
    gd = [dev(t) for t in gains] + [None] * (3 - parts)
    tag = f"headnorm {rows}x{heads} S={S} parts={parts} rope={rope_mask} bf16={bf16}"
    y = Guarded(rows, W, dtype=dt, ld=W + 8)
    kk.call("kk_headnorm_rope_fwd", xd, W, y.t, y.ld, rows, heads, S, parts, *gd, rope_mask, ct, st, bf16)
    torch.cuda.synchronize()
    assert y.intact(), f"{tag}: a guard row / column was written"
    bounded(f"{tag} y", y.t, r32["y"], r64["y"], extra)
    nb = kk.load().kk_headnorm_bwd_blocks(rows, heads)
    assert nb == min(512, -(-rows * heads // 128))
    dxs = []
    for use_part in (0, 1):
        dx = Guarded(rows, W, dtype=dt, ld=W + 8)
        dgs = [gvec(64, 0.0) for _ in range(parts)]
        part = Guarded(parts * nb, 64)
        dgp = [b.t for b in dgs] + [None] * (3 - parts)
        kk.call("kk_headnorm_rope_bwd", dyd, W, xd, W, dx.t, dx.ld, rows, heads, S, parts, *gd, *dgp, part.t if use_part else None,
                rope_mask, ct, st, bf16)
        what = f"{tag} {'partials' if use_part else 'atomics'}"
        if use_part:
            assert all(float(b.t.abs().max()) == 0.0 for b in dgs), f"{what}: with partial rows the launch must not touch dgain"
            assert bool(torch.isfinite(part.t).all()), f"{what}: a partial row was not written"
            table = [(part.t[j * nb:(j + 1) * nb], dgs[j].t, None, nb, 64, 64) for j in range(parts)]
            kk.call("kk_partials_reduce", kk.reduce_table(table, "cuda"), parts, 64)
        torch.cuda.synchronize()
        assert dx.intact() and part.intact() and all(b.intact() for b in dgs), f"{what}: a guard row / column was written"
        bounded(f"{what} dx", dx.t, r32["dx"], r64["dx"], extra)
        for j in range(parts):
            bounded(f"{what} dgain{j}", dgs[j].t[0], r32["dgain"][j], r64["dgain"][j])
        dxs.append(dx.t.clone())
    assert torch.equal(dxs[0], dxs[1])


@pytest.mark.parametrize("bf16", [0, 1])
def test_headnorm_rope_strided_single_part_fp64(kk, bf16):
    """One part of a fused [rows, 3H] projection (the cross-attention q form): x, dy and dx with row strides of their own."""
    rows, heads, S = 131, 3, 44
    H = heads * 64
    g = torch.Generator().manual_seed(5 + bf16)
    xf, dy = torch.randn(rows, 3 * H, generator=g) * 2 + 0.5, torch.randn(rows, H, generator=g)
    if bf16:
        xf, dy = _r16(xf), _r16(dy)
    gain = torch.rand(64, generator=g) + 0.5
    cos, sin = O.rope_tables(S, 64)
    x = xf[:, H:2 * H]
    r32 = _headnorm_ref(x, [gain], dy, cos, sin, heads, S, 1, torch.float32)
    r64 = _headnorm_ref(x, [gain], dy, cos, sin, heads, S, 1, torch.float64)
    dt = torch.bfloat16 if bf16 else torch.float32
    extra = BF16_ROUND if bf16 else 0.0
    xd, ct, st, gd = dev(xf).to(dt), dev(cos), dev(sin), dev(gain)
    dyd = Guarded(rows, H, dtype=dt, fill=dy.cuda().to(dt), ld=H + 4)
    y, dx, dg = Guarded(rows, H, dtype=dt, ld=H + 8), Guarded(rows, H, dtype=dt, ld=2 * H), gvec(64, 0.0)
    kk.call("kk_headnorm_rope_fwd", xd[:, H:], 3 * H, y.t, y.ld, rows, heads, S, 1, gd, None, None, 1, ct, st, bf16)
    kk.call("kk_headnorm_rope_bwd", dyd.t, dyd.ld, xd[:, H:], 3 * H, dx.t, dx.ld, rows, heads, S, 1, gd, None, None, dg.t, None, None,
            None, 1, ct, st, bf16)
    torch.cuda.synchronize()
    assert y.intact() and dx.intact() and dg.intact() and dyd.intact()
    tag = f"headnorm strided single part bf16={bf16}"
    bounded(f"{tag} y", y.t, r32["y"], r64["y"], extra)
    bounded(f"{tag} dx", dx.t, r32["dx"], r64["dx"], extra)
    bounded(f"{tag} dgain", dg.t[0], r32["dgain"][0], r64["dgain"][0])


# ------------------------------------------------------------------ GroupNorm(1, C) per chunk of frames + ReLU
# (B, L, C, chunk): a 1-frame tail (zero output, zero gradient) beside a full chunk | several chunks, 256 / C = 1 frame lane |
# the smallest live chunk: 2 frames of 4 channels
GN_CASES = [(3, 513, 32, 512), (2, 129, 256, 64), (1, 2, 4, 512)]


def _gn_ref(x, gamma, beta, dy, B, L, C, ck, dtype):
    xr = x.to(dtype).view(B, L, C).clone().requires_grad_(True)
    gr, br = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    outs, stats, live = [], [], []
    for c0 in range(0, L, ck):
        xc = xr[:, c0:c0 + ck]
        live.append(xc.shape[1] >= 2)
        if not live[-1]:
            outs.append(torch.zeros_like(xc))
            stats.append(torch.zeros(B, 2, dtype=dtype))
            continue
        mu, var = xc.mean((1, 2), keepdim=True), xc.var((1, 2), unbiased=False, keepdim=True)
        outs.append(torch.relu((xc - mu) / torch.sqrt(var + 1e-5) * gr + br))
        stats.append(torch.stack([mu.reshape(B), (1 / torch.sqrt(var + 1e-5)).reshape(B)], 1).detach())
    y = torch.cat(outs, 1)
    y.backward(dy.to(dtype).view(B, L, C))
    return dict(y=y.detach().view(B * L, C), dx=xr.grad.view(B * L, C), dgamma=gr.grad, dbeta=br.grad,
                stats=torch.stack(stats, 1), live=torch.tensor(live))             # stats [B, nch, 2]


def _gn_inputs(B, L, C):
    g = torch.Generator().manual_seed(B * L + C)
    x = torch.randn(B * L, C, generator=g) * 2 + 0.5
    return x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.randn(B * L, C, generator=g)


@pytest.mark.parametrize("dx_bf16", [0, 1])
@pytest.mark.parametrize("B,L,C,chunk", GN_CASES)
def test_groupnorm_relu_fp64(kk, B, L, C, chunk, dx_bf16):
    """Forward and backward against float64.  The two entry points share one scratch buffer and zero it themselves when they start:
    what a caller leaves in it (NaN here) must not reach any output."""
    x, gamma, beta, dy = _gn_inputs(B, L, C)
    rows, nch = B * L, -(-L // chunk)
    r32, r64 = _gn_ref(x, gamma, beta, dy, B, L, C, chunk, torch.float32), _gn_ref(x, gamma, beta, dy, B, L, C, chunk, torch.float64)
    xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
    tag = f"groupnorm {B}x{L}x{C} chunk={chunk} dx_bf16={dx_bf16}"
    y, st, scr = Guarded(rows, C), Guarded(B * nch, 2), Guarded(1, 2 * B * nch, dtype=torch.float64)
    kk.call("kk_groupnorm_relu_fwd", xd, gd, bd, y.t, st.t, scr.t, None, B, L, C, chunk, None, 0, 0.0)
    torch.cuda.synchronize()
    assert y.intact() and st.intact() and scr.intact(), f"{tag}: a guard row / column was written"
    bounded(f"{tag} y", y.t, r32["y"], r64["y"])
    live = r64["live"]
    got_st = st.t.view(B, nch, 2).cpu()[:, live]
    bounded(f"{tag} mean", got_st[..., 0], r32["stats"][:, live, 0], r64["stats"][:, live, 0])
    bounded(f"{tag} rstd", got_st[..., 1], r32["stats"][:, live, 1], r64["stats"][:, live, 1])
    dead = (~live).nonzero().flatten().tolist()
    yv = y.t.view(B, L, C)
    for ci in dead:
        assert float(yv[:, ci * chunk:(ci + 1) * chunk].abs().max()) == 0.0, f"{tag}: a chunk of one frame gives zeros"
    dx = Guarded(rows, C, dtype=torch.bfloat16 if dx_bf16 else torch.float32)
    dg, db = gvec(C, 0.0), gvec(C, 0.0)
    scr.t.fill_(NAN)
    kk.call("kk_groupnorm_relu_bwd", dyd, xd, y.t, gd, st.t, dx.t, dg.t, db.t, scr.t, B, L, C, chunk, 0.0, dx_bf16)
    torch.cuda.synchronize()
    assert dx.intact() and dg.intact() and db.intact() and scr.intact() and y.intact(), f"{tag}: a guard row / column was written"
    bounded(f"{tag} dx", dx.t, r32["dx"], r64["dx"], BF16_ROUND if dx_bf16 else 0.0)
    bounded(f"{tag} dgamma", dg.t[0], r32["dgamma"], r64["dgamma"])
    bounded(f"{tag} dbeta", db.t[0], r32["dbeta"], r64["dbeta"])
    dxv = dx.t.view(B, L, C)
    for ci in dead:
        assert float(dxv[:, ci * chunk:(ci + 1) * chunk].float().abs().max()) == 0.0, f"{tag}: a chunk of one frame gets no gradient"


@pytest.mark.parametrize("B,L,C,chunk", GN_CASES)
def test_groupnorm_relu_scratch_is_zero_after_use(kk, B, L, C, chunk):
    """The forward and the backward share one float64 scratch: each hands it back zeroed (the forward's finalize pass clears what it
    read, the backward clears it behind its apply pass), beside zeroing it when it starts (test_groupnorm_relu_fp64 poisons it).
    Before they did, the sums stayed in it: max|scratch| after the forward / the backward was 7.2e4 / 90 at (3, 513, 32, 512),
    7.1e4 / 211 at (2, 129, 256, 64), 38.8 / 2.1 at (1, 2, 4, 512)."""
    x, gamma, beta, dy = _gn_inputs(B, L, C)
    rows, nch = B * L, -(-L // chunk)
    xd, gd = dev(x), dev(gamma)
    y, st = torch.empty(rows, C, device="cuda"), torch.empty(B * nch, 2, device="cuda")
    scr = torch.zeros(2 * B * nch, dtype=torch.float64, device="cuda")
    kk.call("kk_groupnorm_relu_fwd", xd, gd, dev(beta), y, st, scr, None, B, L, C, chunk, None, 0, 0.0)
    after_fwd = float(scr.abs().max())
    dx, dg, db = torch.empty(rows, C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    kk.call("kk_groupnorm_relu_bwd", dev(dy), xd, y, gd, st, dx, dg, db, scr, B, L, C, chunk, 0.0, 0)
    after_bwd = float(scr.abs().max())
    print(f"[norm-fp64] groupnorm {B}x{L}x{C} chunk={chunk}: max|scratch| after fwd {after_fwd:.3e}, after bwd {after_bwd:.3e}")
    assert after_fwd == 0.0 and after_bwd == 0.0, (after_fwd, after_bwd)


@pytest.mark.parametrize("B,L,C,chunk", GN_CASES)
def test_groupnorm_relu_dropout_backward_equals_explicit_mask(kk, B, L, C, chunk):
    """p > 0: the backward only needs 1/(1-p), because dropped elements are stored as zeros — it equals the p = 0 backward of the
    masked dy (the mask stream itself is checked in test_kernels_gpu.py)."""
    x, gamma, beta, dy = _gn_inputs(B, L, C)
    rows, nch, p = B * L, -(-L // chunk), 0.1
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    y0, y1, st = torch.empty(rows, C, device="cuda"), torch.empty(rows, C, device="cuda"), torch.empty(B * nch, 2, device="cuda")
    scr = torch.zeros(2 * B * nch, dtype=torch.float64, device="cuda")
    seed = torch.tensor([1234], dtype=torch.int32, device="cuda")
    kk.call("kk_groupnorm_relu_fwd", xd, gd, bd, y0, st, scr, None, B, L, C, chunk, None, 0, 0.0)
    kk.call("kk_groupnorm_relu_fwd", xd, gd, bd, y1, st, scr, None, B, L, C, chunk, seed, 2, p)
    pos = y0 > 1e-6
    ratio = (y1[pos] / y0[pos]).cpu()
    assert bool(((ratio.abs() < 1e-5) | ((ratio - 1 / (1 - p)).abs() < 1e-4)).all()), "mask values must be 0 or 1/keep"
    keep = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))                       # the kernels' 1.f / (1.f - p)
    mask = torch.where(y0 > 0, (y1 > 0).float() * keep.cuda(), torch.ones_like(y0)).cpu()
    a0, a1 = torch.empty(rows, C, device="cuda"), torch.empty(rows, C, device="cuda")
    gg0, gb0, gg1, gb1 = (torch.zeros(C, device="cuda") for _ in range(4))
    kk.call("kk_groupnorm_relu_bwd", dev(dy * mask), xd, y0, gd, st, a0, gg0, gb0, scr, B, L, C, chunk, 0.0, 0)
    kk.call("kk_groupnorm_relu_bwd", dev(dy), xd, y1, gd, st, a1, gg1, gb1, scr, B, L, C, chunk, p, 0)
    for got, ref, atol, what in ((a1, a0, 1e-5, "dx"), (gg1, gg0, 1e-4, "dgamma"), (gb1, gb0, 1e-4, "dbeta")):
        err = (got - ref).abs()
        assert bool((err <= atol + 1e-4 * ref.abs()).all()), f"groupnorm dropout backward {what}: max|err| = {float(err.max()):.3e}"
