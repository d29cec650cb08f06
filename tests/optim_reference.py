"""Shared by test_optim_reference_cpu.py and test_optim_kernels_gpu.py: plain restatements of the optimizer pass (kk_optim.hip) and
the inputs both files use.  Not a test.

The restatements are written from the formulas (torch.optim.AdamW with decoupled decay, the EMA, the Q34.30 norm accumulator, the
weight-norm projection), not from the kernels' instruction order; opt_prepare_ref alone is a replay, because the step driver's state
machine IS its order of statements.  test_optim_reference_cpu.py ties them to torch.optim.AdamW and to the step-driver goldens.

What counts as an input.  The C ABI takes beta1, beta2 and ema_decay as floats and gscale / decay / stepsize / consts as fp32 arrays:
the fp32 values are the inputs, and the references start from them (1 - float32(0.999) is not 0.001; with the rounded value both
1 - beta are exact in fp32 and in fp64, so the restatements differ in arithmetic only, never in constants)."""
import functools
import math

import numpy as np
import torch

from kokoro_ruslan_amd.lib import OS, KkOptCfg

BLK = 1024                               # KK_SEG_ALIGN: elements per arena block
Q30 = 2.0 ** 30                          # p_sumsq is a Q34.30 fixed-point sum
PSUMSQ_CLAMP = 2.0 ** 22                 # a block's share of p_sumsq is clamped to this
SEG_SUMSQ_WGS = 2048                     # kk_seg_sumsq always launches this many workgroups: per = ceil(nblocks / 2048) blocks each
WNP_BLOCKS = 8                           # kk_weight_norm_project: arena blocks per workgroup


def f32(x):
    """The fp32 value of a scalar, as a Python float."""
    return float(np.float32(x))


def elem_seg(block_seg):
    return torch.as_tensor(block_seg).long().repeat_interleave(BLK)


# ------------------------------------------------------------------------------------------------ AdamW + EMA
def adamw_ema_ref(p, g, m, v, ema, block_seg, gscale, decay, stepsize, flags, consts, beta1, beta2, ema_decay, dtype=torch.float64,
                  variant=None):
    """One kk_adamw_ema pass over the arena in `dtype` (float64: the reference; float32: the restatement fp64_bounds.bounded wants).
    consts = [mode, sqrt(1 - beta2^k), eps, ...]; mode 0: step and EMA, 1: nothing, 2: step without EMA.  flags per segment: bit 0 step,
    bit 1 EMA tracked.  ema may be None.  Returns p, m, v, ema in `dtype`.  `variant` selects one of MUTANTS (None: the true formulas)."""
    assert variant is None or variant in MUTANT_NAMES, variant
    es = elem_seg(block_seg)
    per = lambda t: torch.as_tensor(t)[es]                                    # noqa: E731  (per-segment table -> per element)
    T = lambda t: torch.as_tensor(t).to(dtype)                                # noqa: E731
    p0, g0, m0, v0 = T(p), T(g), T(m), T(v)
    e0 = None if ema is None else T(ema)
    gs, dc, st = T(per(gscale)), T(per(decay)), T(per(stepsize))
    fl = per(flags).long()
    mode, bc2s, eps = float(consts[0]), float(consts[1]), float(consts[2])
    b1, b2, d = f32(beta1), f32(beta2), f32(ema_decay)
    stepping = (mode != 1.0) or variant == "mode1_writes"
    ema_moves = (mode == 0.0) or (mode == 2.0 and variant == "ema_in_mode2") or variant == "mode1_writes"

    gr = g0 * gs
    if variant == "coupled_l2":                                               # g += wd p  (lr wd = 1 - decay), no decay of p
        gr = gr + (1.0 - dc) / torch.where(st > 0, st, torch.ones_like(st)) * p0
    if variant == "beta1_swapped":
        m1 = (1.0 - b1) * m0 + b1 * gr
    else:
        m1 = b1 * m0 + (1.0 - b1) * gr
    if variant == "v_without_gscale":
        v1 = b2 * v0 + (1.0 - b2) * g0 * g0
    else:
        v1 = b2 * v0 + (1.0 - b2) * gr * gr
    vd = v0 if variant == "denom_from_old_v" else v1
    if variant == "eps_inside_sqrt":
        denom = torch.sqrt(vd + eps) / bc2s
    elif variant == "bc2_inside_sqrt":
        denom = torch.sqrt(vd / bc2s) + eps
    else:
        denom = torch.sqrt(vd) / bc2s + eps
    upd = st * ((m0 if variant == "update_from_old_m" else m1) / denom)
    if variant == "coupled_l2":
        p1 = p0 - upd
    elif variant == "decay_after_step":
        p1 = (p0 - upd) * dc
    else:
        p1 = p0 * dc - upd
    step = ((fl & 1) != 0) & stepping
    p_new, m_new, v_new = torch.where(step, p1, p0), torch.where(step, m1, m0), torch.where(step, v1, v0)
    e_new = None
    if e0 is not None:
        src = p0 if variant == "ema_from_old_p" else p_new
        e_new = torch.where(((fl & 2) != 0) & ema_moves, d * e0 + (1.0 - d) * src, e0)
    return p_new, m_new, v_new, e_new


# deliberately wrong variants of adamw_ema_ref, one line each: test_optim_reference_cpu.py shows that the GPU suite's inputs and bound
# tell every one of them from the true formulas
MUTANT_NAMES = ("eps_inside_sqrt", "bc2_inside_sqrt", "coupled_l2", "decay_after_step", "v_without_gscale", "beta1_swapped",
                "update_from_old_m", "denom_from_old_v", "ema_from_old_p", "ema_in_mode2", "mode1_writes")
MUTANTS = {name: functools.partial(adamw_ema_ref, variant=name) for name in MUTANT_NAMES}


# the arena of the kk_adamw_ema value tests: 9 segments, 40 blocks; `ragged` is the logical length inside each segment's last block
ADAMW_FLAGS = [3, 1, 2, 0, 7, 4, 6, 5, 3]
ADAMW_LENS = [5, 1, 7, 3, 6, 1, 4, 8, 5]
ADAMW_RAGGED = [1, 513, 1023, 7, 300, 1, 1000, 77, 640]
ADAMW_GSCALE = [0.37, 1.0, 1.0, 0.37, 1.0, 0.0, 0.37, 0.0, 0.37]
ADAMW_DECAY = [0.999, 1.0 - 1e-6, 1.0, 0.999, 0.999, 1.0, 1.0 - 1e-6, 1.0, 1.0]
ADAMW_STEPSIZE = dict(sharp=[1e-2, 3e-7, 1e-2, 0.0, 1e-2, 1e-2, 0.0, 1e-2, 0.0],
                      realistic=[3e-7, 3e-7, 1e-2, 0.0, 3e-7, 0.0, 3e-7, 1e-2, 0.0])
ADAMW_EMA_DECAY = dict(sharp=0.9, realistic=0.9999)
ADAMW_BETAS = (0.9, 0.999)
ADAMW_K = 7                                                                    # successful steps so far: bc2s = sqrt(1 - beta2^8) = 0.089


def seg_layout(lens):
    """block_seg (int32 [nblocks]) and each segment's first block for segments of `lens` blocks."""
    lens = torch.as_tensor(lens, dtype=torch.long)
    block_seg = torch.repeat_interleave(torch.arange(len(lens), dtype=torch.int32), lens)
    first = torch.cumsum(lens, 0) - lens
    return block_seg, [int(x) for x in first]


def seg_slices(lens):
    _, first = seg_layout(lens)
    return [slice(f * BLK, (f + int(n)) * BLK) for f, n in zip(first, lens)]


@functools.lru_cache(maxsize=None)
def adamw_case(regime):
    """Inputs of the kk_adamw_ema value tests (CPU fp32 tensors; do not modify: shared between tests).
    sharp: |p| ~ 1e-3 under steps of 1e-2 with |g| from 1e-9 to 1 — the step and the EMA delta are as large as what they are added
    to; realistic: |p| ~ 1, lr-sized steps, ema_decay 0.9999.  Every 16th element of a segment is, in turn: g = 0 | m = v = 0 |
    v an fp32 denormal | g, m, v so small that eps decides denom.  Past each segment's ragged logical length everything is zero."""
    gen = torch.Generator().manual_seed(dict(sharp=101, realistic=202)[regime])
    n = sum(ADAMW_LENS) * BLK
    rn = lambda: torch.randn(n, generator=gen)                                # noqa: E731
    ru = lambda: torch.rand(n, generator=gen)                                 # noqa: E731
    if regime == "sharp":
        gmag = 10.0 ** (-9.0 * ru())
        p, ema = 1e-3 * rn(), 1e-3 * rn()
    else:
        gmag = 10.0 ** (-4.0 + 3.0 * ru())
        p = rn()
        ema = p + 1e-3 * rn()
    g = gmag * torch.sign(rn())
    m = 2.0 * gmag * rn()
    v = (gmag * (0.5 + ru())) ** 2
    block_seg, _ = seg_layout(ADAMW_LENS)
    for sl, nb, r in zip(seg_slices(ADAMW_LENS), ADAMW_LENS, ADAMW_RAGGED):
        i = torch.arange(nb * BLK) % 16
        gs, ms, vs = g[sl], m[sl], v[sl]                                      # (views)
        gs[i == 3] = 0.0
        ms[i == 5] = 0.0
        vs[i == 5] = 0.0
        vs[i == 7] = 3e-40                                                    # an fp32 denormal, under a gradient whose square underflows
        gs[i == 7] *= 1e-12
        ms[i == 7] *= 1e-12
        gs[i == 9] = 1e-11 * torch.sign(gs[i == 9])                           # sqrt(v) / bc2s ~ 1e-10 << eps = 1e-8, m / eps = 0.2
        ms[i == 9] = 2e-9 * torch.sign(ms[i == 9])
        vs[i == 9] = 1e-22
        for t in (p, g, m, v, ema):
            t[sl][(nb - 1) * BLK + r:] = 0.0
    assert float(v.min()) >= 0.0 and 0.0 < float(v[v > 0].min()) < 1.1754944e-38
    b1, b2 = ADAMW_BETAS
    consts = torch.tensor([0.0, math.sqrt(1.0 - f32(b2) ** (ADAMW_K + 1)), 1e-8, 1e-4], dtype=torch.float32)
    return dict(p=p, g=g, m=m, v=v, ema=ema, block_seg=block_seg, nblocks=len(block_seg), nseg=len(ADAMW_LENS),
                flags=torch.tensor(ADAMW_FLAGS, dtype=torch.int32), gscale=torch.tensor(ADAMW_GSCALE, dtype=torch.float32),
                decay=torch.tensor(ADAMW_DECAY, dtype=torch.float32),
                stepsize=torch.tensor(ADAMW_STEPSIZE[regime], dtype=torch.float32), consts=consts, beta1=b1, beta2=b2,
                ema_decay=ADAMW_EMA_DECAY[regime], slices=seg_slices(ADAMW_LENS))


def adamw_refs(regime, mode, with_ema=True, variant=None, dtype=torch.float64):
    """(p, m, v, ema) of adamw_case(regime) at `mode`."""
    c = adamw_case(regime)
    consts = c["consts"].clone()
    consts[0] = float(mode)
    return adamw_ema_ref(c["p"], c["g"], c["m"], c["v"], c["ema"] if with_ema else None, c["block_seg"], c["gscale"], c["decay"],
                         c["stepsize"], c["flags"], consts, c["beta1"], c["beta2"], c["ema_decay"], dtype, variant=variant)


def written(flags, mode, what, with_ema=True):
    """Does kk_adamw_ema write output `what` ('p', 'm', 'v', 'ema') of a segment with these flags at this mode?"""
    if what == "ema":
        return bool(flags & 2) and mode == 0 and with_ema
    return bool(flags & 1) and mode != 1


# ------------------------------------------------------------------------------------------------ norm accumulators, projection
def p_sumsq_ref(p, block_seg, flags, nseg):
    """Q34.30 sums of squares of the flag-bit-2 segments (int64 [nseg], zero elsewhere): each 1024-element block contributes
    round(min(s, 2^22) 2^30), s its sum of squares; a NaN block counts as the clamp."""
    s = torch.as_tensor(p).double().view(-1, BLK).square().sum(1).numpy()
    out = [0] * nseg
    for b, sg in enumerate(torch.as_tensor(block_seg).tolist()):
        if int(flags[sg]) & 4:
            sc = PSUMSQ_CLAMP if not (s[b] < PSUMSQ_CLAMP) else float(s[b])
            out[sg] += int(math.floor(sc * Q30 + 0.5))
    return torch.tensor(out, dtype=torch.int64)


def seg_sumsq_ref(buf, block_seg, nseg):
    """(float64 [nseg] sums of squares, bool [nseg] 'owns a block').  A segment id without a block is not stored by kk_seg_sumsq."""
    s = torch.as_tensor(buf).double().view(-1, BLK).square().sum(1)
    bs = torch.as_tensor(block_seg).long()
    out = torch.zeros(nseg, dtype=torch.float64).index_add_(0, bs, s)
    owned = torch.zeros(nseg, dtype=torch.bool)
    owned[bs] = True
    return out, owned


def project_ref(p, block_seg, p_sumsq, flags, mode, max_norm):
    """kk_weight_norm_project: (p in float64 after the projection, bool per block 'rewritten').  A flag-bit-2 segment whose norm
    sqrt(p_sumsq / 2^30) is strictly above max_norm is multiplied by float32(max_norm / norm)."""
    out = torch.as_tensor(p).double().clone()
    bs = torch.as_tensor(block_seg).tolist()
    moved = torch.zeros(len(bs), dtype=torch.bool)
    if mode == 1 or not max_norm > 0.0:
        return out, moved
    for b, sg in enumerate(bs):
        if int(flags[sg]) & 4:
            nr = math.sqrt(int(p_sumsq[sg]) / Q30)
            if nr > max_norm:
                out[b * BLK:(b + 1) * BLK] *= f32(max_norm / nr)
                moved[b] = True
    return out, moved


# ------------------------------------------------------------------------------------------------ the step driver
def make_cfg(**over):
    """A KkOptCfg with quiet defaults (no warm-up, explosion floor out of reach, short mel: no adaptive clip)."""
    c = KkOptCfg()
    c.learning_rate, c.max_lr, c.warmup_start_lr, c.warmup_target_lr, c.use_warmup = 1e-3, 1e-3, 1e-4, 1e-3, 0
    c.pct_start, c.div_factor, c.final_div_factor, c.warmup_steps, c.onecycle_steps = 0.3, 25.0, 1e4, 10, 1000
    c.max_grad_norm, c.beta1, c.beta2, c.eps, c.mel_length = 1.0, 0.9, 0.999, 1e-8, 64
    c.expl_abs_floor, c.expl_warmup_floor, c.expl_multiplier, c.expl_alpha = 1e9, 1e9, 10.0, 0.9
    c.expl_warmup_steps, c.expl_min_ema_steps, c.ema_decay, c.max_weight_norm = 0, 5, 0.999, 0.0
    c.ema_update_every, c.legacy_schedule, c.legacy_cos, c.eta_min = 1, 0, 0.0, 1e-6
    for k, val in over.items():
        assert hasattr(c, k), k
        setattr(c, k, val)
    return c


def cfg_from_hyper(hp, total_steps, mel_length):
    """The KkOptCfg the engine builds from a spec.StepHyper (engine.KokoroEngine._opt_cfg, one-cycle schedule)."""
    from kokoro_ruslan_amd import spec
    c = spec.lr_schedule_consts(hp, total_steps)
    return KkOptCfg(c["learning_rate"], c["max_lr"], c["warmup_start_lr"], c["warmup_target_lr"], c["pct_start"], c["div_factor"],
                    c["final_div_factor"], c["warmup_steps"], c["onecycle_steps"], c["use_warmup"], hp.adam_betas[0], hp.adam_betas[1],
                    hp.adam_eps, hp.max_grad_norm, mel_length, hp.grad_explosion_ema_alpha, hp.grad_explosion_abs_floor,
                    hp.grad_explosion_multiplier, hp.grad_explosion_warmup_floor, hp.grad_explosion_warmup_steps,
                    hp.grad_explosion_min_ema_steps, hp.ema_decay, hp.dec_ffn_max_weight_norm, max(1, int(hp.ema_update_every)),
                    0, 0.0, hp.lr_eta_min)


def _onecycle_lr(c, step_num):
    total = float(c.onecycle_steps)
    initial = c.max_lr / c.div_factor
    min_lr = initial / c.final_div_factor
    end1, end2 = c.pct_start * total - 1.0, total - 1.0
    if step_num <= end1:
        if end1 <= 0:
            return c.max_lr
        return (initial - c.max_lr) / 2.0 * (math.cos(math.pi * (step_num / end1)) + 1.0) + c.max_lr
    if end2 <= end1:
        return min_lr
    return (c.max_lr - min_lr) / 2.0 * (math.cos(math.pi * ((step_num - end1) / (end2 - end1))) + 1.0) + min_lr


def base_lr_ref(c, k):
    """Base LR of successful step k (0-based): linear warm-up, then torch's OneCycleLR (cosine, two phases)."""
    if k == 0:
        return _onecycle_lr(c, 0)
    j = k - 1
    if c.use_warmup and j < c.warmup_steps:
        return c.warmup_start_lr + (c.warmup_target_lr - c.warmup_start_lr) * (j / c.warmup_steps)
    s = j - c.warmup_steps + 1 if c.use_warmup else j + 1
    return _onecycle_lr(c, min(s, c.onecycle_steps))


def opt_prepare_ref(grad_sumsq, seg_preclip, seg_lr_mult, seg_wd, cfg, state, max_dur=0):
    """Host replay of opt_prepare_kernel in float64, fp32 casts included.  `state` is the 16-double state vector on entry.
    Returns dict(st, gscale, decay, stepsize, consts) (float64 state, fp32 arrays)."""
    c = cfg
    ss = np.asarray(grad_sumsq, dtype=np.float64)
    pre = np.asarray(seg_preclip, dtype=np.float32).astype(np.float64)
    mult = np.asarray(seg_lr_mult, dtype=np.float32).astype(np.float64)
    wd = np.asarray(seg_wd, dtype=np.float32).astype(np.float64)
    st = np.array(state, dtype=np.float64)
    fin = np.isfinite(ss)
    with np.errstate(invalid="ignore"):
        nr = np.sqrt(ss)
        sc = np.where((pre > 0.0) & fin & (nr > pre), pre / (nr + 1e-12), 1.0)
        gs0 = sc.astype(np.float32)                                           # provisional: the pre-clip factor, stored as fp32
        total = math.sqrt(float(np.sum((nr * sc) ** 2)))
    nbad = int((~fin).sum())
    clip = c.max_grad_norm
    risk = max(c.mel_length / 1400.0, float(max_dur) / 150.0)
    if risk > 1.0:
        clip = min(clip, max(0.3, 0.8 / risk ** 0.35))
        clip = max(0.05, 0.5 / math.sqrt(risk))
    attempt = st[OS["ATTEMPT"]]
    done = attempt - st[OS["SKIPPED"]]
    floor_ = c.expl_abs_floor
    if c.expl_warmup_steps > 0 and done < c.expl_warmup_steps:
        floor_ = c.expl_warmup_floor - (c.expl_warmup_floor - c.expl_abs_floor) * (done / c.expl_warmup_steps)
    ema_valid = st[OS["EXPL_EMA_VALID"]] != 0.0
    ema_ready = st[OS["EXPL_EMA_STEPS"]] >= c.expl_min_ema_steps
    ema_thr = st[OS["EXPL_EMA"]] * c.expl_multiplier if ema_valid else 0.0
    thr = (ema_thr if ema_thr > floor_ else floor_) if ema_ready else floor_     # fmax: a NaN operand loses
    if total > thr:
        st[OS["EXPL_STREAK"]] += 1.0
        clip = min(clip, 0.3)
    else:
        st[OS["EXPL_STREAK"]] = 0.0
    st[OS["EXPL_EMA"]] = c.expl_alpha * st[OS["EXPL_EMA"]] + (1.0 - c.expl_alpha) * total if ema_valid else total
    st[OS["EXPL_EMA_VALID"]] = 1.0
    st[OS["EXPL_EMA_STEPS"]] += 1.0
    skip = nbad > 0 or st[OS["MICRO_BAD"]] != 0.0
    st[OS["MICRO_BAD"]] = 0.0
    k = int(done)
    r = clip / (total + 1e-6)
    coef = r if r < 1.0 else 1.0                                              # fmin(1, NaN) = 1
    blr = c.eta_min + (c.learning_rate - c.eta_min) * c.legacy_cos if c.legacy_schedule else base_lr_ref(c, k)
    bc1 = 1.0 - c.beta1 ** (k + 1)
    consts = np.zeros(4, dtype=np.float32)
    consts[0] = 1.0 if skip else (2.0 if c.ema_update_every > 1 and k % c.ema_update_every != 0 else 0.0)
    consts[1] = np.float32(math.sqrt(1.0 - c.beta2 ** (k + 1)))
    consts[2] = np.float32(c.eps)
    consts[3] = np.float32(blr)
    st[OS["ATTEMPT"]] = attempt + 1.0
    if skip:
        st[OS["SKIPPED"]] += 1.0
        st[OS["BAD_SEG"]] = float(int(np.argmax(~fin)) + 1) if nbad else float(0x7fffffff + 1)
        st[OS["BAD_COUNT"]] = float(nbad)
        st[OS["BAD_ATTEMPT"]] = attempt
    st[OS["LAST_GRAD_NORM"]] = total
    st[OS["LAST_CLIP_COEF"]] = coef
    st[OS["LAST_SKIP"]] = 1.0 if skip else 0.0
    st[OS["LAST_BASE_LR"]] = blr
    st[OS["LAST_CLIP_NORM"]] = clip
    if c.legacy_schedule:
        lr = c.eta_min + (c.learning_rate * mult - c.eta_min) * c.legacy_cos
    else:
        lr = blr * mult
    with np.errstate(invalid="ignore"):
        gscale = (gs0.astype(np.float64) * coef).astype(np.float32)
    return dict(st=st, gscale=gscale, decay=(1.0 - lr * wd).astype(np.float32), stepsize=(lr / bc1).astype(np.float32), consts=consts)
