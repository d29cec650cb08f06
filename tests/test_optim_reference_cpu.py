"""CPU suite: the references of tests/optim_reference.py against what the project did not write (torch.optim.AdamW, the step-driver
goldens recorded from the reference's own statements), and the proof that the inputs of test_optim_kernels_gpu.py tell a subtly wrong
AdamW from the right one at that file's acceptance bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_reference as R  # noqa: E402
from fp64_bounds import FLOOR, nerr  # noqa: E402

OS = R.OS


def test_adamw_ema_ref_is_torch_adamw():
    """3 steps of a two-tensor problem in float64: adamw_ema_ref fed decay = 1 - lr wd, stepsize = lr / (1 - beta1^k) and
    bc2s = sqrt(1 - beta2^k) — the way opt_prepare_kernel derives them — gives torch.optim.AdamW's weights and moments to 1e-12."""
    gen = torch.Generator().manual_seed(3)
    sizes, lens = [700, 1500], [1, 2]
    lrs, wds = [3e-3, 1e-2], [0.05, 0.0]
    b1, b2, eps = R.f32(0.9), R.f32(0.999), 1e-8                              # (the ABI's betas are floats: fp32 values on both sides)
    block_seg, first = R.seg_layout(lens)
    n = sum(lens) * R.BLK
    views = [slice(f * R.BLK, f * R.BLK + s) for f, s in zip(first, sizes)]
    p, m, v = (torch.zeros(n, dtype=torch.float64) for _ in range(3))
    for sl in views:
        p[sl] = torch.randn(sl.stop - sl.start, generator=gen, dtype=torch.float64)
    params = [torch.nn.Parameter(p[sl].clone()) for sl in views]
    opt = torch.optim.AdamW([dict(params=[q], lr=lr, weight_decay=wd) for q, lr, wd in zip(params, lrs, wds)], betas=(b1, b2), eps=eps)
    flags = torch.tensor([1, 1], dtype=torch.int32)
    for k in range(3):
        g = torch.zeros(n, dtype=torch.float64)
        for sl, q in zip(views, params):
            g[sl] = torch.randn(sl.stop - sl.start, generator=gen, dtype=torch.float64) * 10.0 ** (-k)
            q.grad = g[sl].clone()
        opt.step()
        bc1 = 1.0 - b1 ** (k + 1)
        consts = [0.0, math.sqrt(1.0 - b2 ** (k + 1)), eps, 0.0]
        decay = torch.tensor([1.0 - lr * wd for lr, wd in zip(lrs, wds)], dtype=torch.float64)
        stepsize = torch.tensor([lr / bc1 for lr in lrs], dtype=torch.float64)
        p, m, v, _ = R.adamw_ema_ref(p, g, m, v, None, block_seg, torch.ones(2, dtype=torch.float64), decay, stepsize, flags, consts,
                                     b1, b2, 0.5, torch.float64)
        for sl, q in zip(views, params):
            state = opt.state[q]
            for what, got, want in (("p", p[sl], q.detach()), ("m", m[sl], state["exp_avg"]), ("v", v[sl], state["exp_avg_sq"])):
                rel = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
                assert rel <= 1e-12, (k, what, rel)
        pad = torch.ones(n, dtype=torch.bool)
        for sl in views:
            pad[sl] = False
        assert not bool(p[pad].any() or m[pad].any() or v[pad].any()), "zero padding stays zero"


def _hyper(**kw):
    from kokoro_ruslan_amd import spec
    return spec.StepHyper(gradient_accumulation_steps=1, **kw)


def test_opt_prepare_ref_reproduces_the_explosion_rows(golden_dir):
    """520 scripted gradient norms of step_driver.npz: threshold, emergency clip, EMA and streak, to the tolerances of
    test_engine_gpu.py::test_device_step_driver_against_reference_sequences."""
    rows = np.load(os.path.join(golden_dir, "step_driver.npz"))["explosion"]
    cfg = R.cfg_from_hyper(_hyper(), 20000, 64)
    nseg, seg = 5, 3
    st = np.zeros(OS["SIZE"])
    zero, one = np.zeros(nseg, dtype=np.float32), np.ones(nseg, dtype=np.float32)
    for k, (norm, thr, clip, expl, ema, streak) in enumerate(rows):
        ss = np.zeros(nseg)
        ss[seg] = float(norm) ** 2
        st = R.opt_prepare_ref(ss, zero, one, zero, cfg, st)["st"]
        assert abs(st[OS["LAST_GRAD_NORM"]] - norm) <= 1e-9 * norm
        assert abs(st[OS["LAST_CLIP_NORM"]] - clip) < 1e-12, (k, st[OS["LAST_CLIP_NORM"]], clip)
        assert abs(st[OS["EXPL_EMA"]] - ema) <= 1e-9 * abs(ema) and st[OS["EXPL_STREAK"]] == streak, (k, st, rows[k])
        assert abs(st[OS["LAST_CLIP_COEF"]] - min(1.0, clip / (norm + 1e-6))) < 1e-9
    assert st[OS["ATTEMPT"]] == len(rows) and st[OS["SKIPPED"]] == 0


def test_opt_prepare_ref_reproduces_the_adaptive_clip_rows(golden_dir):
    """The batch-shape clip norms of step_driver.npz (mel length, longest phoneme -> clip), under a gradient too small to explode."""
    rows = np.load(os.path.join(golden_dir, "step_driver.npz"))["adaptive"]
    assert len(rows) > 0
    z, o = np.zeros(1, dtype=np.float32), np.ones(1, dtype=np.float32)
    for mel_len, max_dur, _, clip in rows:
        cfg = R.cfg_from_hyper(_hyper(), 20000, int(mel_len))
        st = R.opt_prepare_ref(np.array([1e-12]), z, o, z, cfg, np.zeros(OS["SIZE"]), max_dur=int(max_dur))["st"]
        assert abs(st[OS["LAST_CLIP_NORM"]] - clip) < 1e-9, (mel_len, max_dur, st[OS["LAST_CLIP_NORM"]], clip)


def test_opt_prepare_ref_reproduces_the_lr_sequence(golden_dir):
    """20 warm-up steps, 40 one-cycle steps and 3 beyond the end against lr_seq_60_20.npy, per parameter group."""
    from kokoro_ruslan_amd import spec
    seq = np.load(os.path.join(golden_dir, "lr_seq_60_20.npy"))
    hp = _hyper(warmup_steps=20)
    cfg = R.cfg_from_hyper(hp, 60, 64)
    table = spec.group_lr_mult_wd(hp)
    mult = np.array([t[0] for t in table], dtype=np.float32)
    wd = np.array([t[1] for t in table], dtype=np.float32)
    st = np.zeros(OS["SIZE"])
    for k in range(len(seq)):
        out = R.opt_prepare_ref(np.full(10, 0.1), np.zeros(10, dtype=np.float32), mult, wd, cfg, st)
        st = out["st"]
        bc1 = 1.0 - hp.adam_betas[0] ** (k + 1)
        for gi in range(10):
            want = float(seq[k, gi])
            assert abs(st[OS["LAST_BASE_LR"]] * table[gi][0] - want) <= 1e-12 + 1e-9 * want, (k, gi)
            assert abs(float(out["stepsize"][gi]) - want / bc1) <= 2e-7 * want / bc1 + 1e-15, (k, gi)
            assert abs(float(out["decay"][gi]) - (1.0 - want * float(wd[gi]))) <= 2.0 ** -23, (k, gi)
        assert float(out["consts"][0]) == 0.0 and abs(float(out["consts"][3]) - st[OS["LAST_BASE_LR"]]) <= 1e-7 * st[OS["LAST_BASE_LR"]]


def test_accumulator_references_round_like_the_kernels_contract():
    """p_sumsq_ref: round-half-up of s 2^30, the 2^22 clamp, NaN as the clamp, nothing for unflagged segments; seg_sumsq_ref marks ids
    that own no block."""
    lens = [1, 1, 1, 1, 1, 2]
    block_seg, _ = R.seg_layout(lens)
    p = torch.zeros(sum(lens) * R.BLK)
    p[0] = 2.0 ** -16                                                         # s = 2^-32: s 2^30 + 0.5 < 1
    p[R.BLK:R.BLK + 2] = 2.0 ** -16                                           # s = 2^-31: exactly one half, rounds up
    p[2 * R.BLK:3 * R.BLK] = 128.0                                            # s = 2^24 > 2^22
    p[3 * R.BLK + 9] = float("nan")
    p[4 * R.BLK:5 * R.BLK] = 1.0                                              # unflagged
    p[5 * R.BLK:7 * R.BLK] = 0.5
    got = R.p_sumsq_ref(p, block_seg, [4, 4, 4, 4, 3, 7], 6)
    assert got.tolist()[:2] == [0, 1] and got.tolist()[2:5] == [2 ** 52, 2 ** 52, 0] and int(got[5]) == 512 * 2 ** 30
    s, owned = R.seg_sumsq_ref(p.nan_to_num(0.0), torch.tensor([0, 1, 2, 3, 4, 6, 6]), 8)
    assert owned.tolist() == [True] * 5 + [False, True, False] and float(s[6]) == 512.0 and float(s[2]) == 2.0 ** 24


@pytest.mark.parametrize("name", R.MUTANT_NAMES)
def test_gpu_inputs_discriminate_every_mutant(name):
    """On the inputs test_optim_kernels_gpu.py feeds kk_adamw_ema, a kernel computing MUTANTS[name] instead of AdamW would miss that
    file's bound, 4 E_ref + 2^-22 per segment and output, by a factor of at least 100 on some checked output.  The factor is a
    condition on the inputs: if a mutant does not clear it, the inputs are too tame."""
    best, where = 0.0, None
    for regime in ("sharp", "realistic"):
        c = R.adamw_case(regime)
        for mode in (0, 1, 2):
            ref64 = R.adamw_refs(regime, mode)
            ref32 = R.adamw_refs(regime, mode, dtype=torch.float32)
            mut = R.adamw_refs(regime, mode, variant=name)
            for what, r64, r32, mu in zip("p m v ema".split(), ref64, ref32, mut):
                for si, sl in enumerate(c["slices"]):
                    bound = 4.0 * nerr(r32[sl], r64[sl]) + FLOOR
                    ratio = nerr(mu[sl], r64[sl]) / bound
                    if ratio > best:
                        best, where = ratio, (regime, mode, what, si)
    print(f"[optim-mutant] {name}: off by {best:.3g} x the bound at {where}")
    assert best >= 100.0, (name, best, where)


def test_true_formulas_pass_their_own_bound():
    """The fp32 restatement differs from float64 by rounding only (E_ref is a few fp32 ulps on every segment and output), and what
    the flags and the mode leave unwritten comes back bit-identical from the reference."""
    for regime in ("sharp", "realistic"):
        c = R.adamw_case(regime)
        for mode in (0, 1, 2):
            ref64 = R.adamw_refs(regime, mode)
            ref32 = R.adamw_refs(regime, mode, dtype=torch.float32)
            for what, r64, r32 in zip("p m v ema".split(), ref64, ref32):
                for si, sl in enumerate(c["slices"]):
                    e = nerr(r32[sl], r64[sl])
                    assert e <= 2.0 ** -20, (regime, mode, what, si, e)
                    if not R.written(R.ADAMW_FLAGS[si], mode, what):
                        assert torch.equal(r32[sl], c[what][sl]) and torch.equal(r64[sl], c[what][sl].double())
