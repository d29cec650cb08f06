"""The loss boundary (csrc/kk_loss.hip: kk_losses_fwd / kk_losses_finalize / kk_losses_bwd) and the two pad / mask kernels beside it
(csrc/kk_elem.hip: kk_frame_mask, kk_pad2d_f32) against a plain fp64 restatement written in this file, on every branch the kernels have.

The reference (`ref_*` below) restates the loss semantics in fp64 torch on the upcast fp32 inputs and never calls O.losses / O.loss_sums:
mel L1 over (frame < mel_len, element finite); duration Huber on (pred, log(d + 1)) over (pos < ph_len, d > 0) with NO finite filter;
stop BCE-with-logits(pos_weight), pitch and energy Huber over (frame < mel_len, term finite); means clamped at 100 / 100 / 100 / 10 / 10
after the mean; coefficient w_k * scale / count_k, 0 above the cap or at count 0; scale = loss_scale * max(0.25, 1 / risk) when
risk = max(T / 1400, max_dur / 150) > 1 and `adaptive` is set.  `test_reference_self_check` (CPU) holds its closed-form gradients to fp64
autograd of its own forward and its forward to O.losses.

Soft stop targets do occur: the data set's targets end in a tail 2^-6 .. 2^-1, 1 (O.stop_targets), so the backward's two BCE terms
partly cancel in every utterance; the planted inputs mix hard 0 / 1 with soft targets under ordinary and saturated logits.

Bounds (none taken from the kernels' own output):
  * six loss scalars and five sums: at most 4x the error of fp32 O.losses / O.loss_sums on the same input against the reference,
    floor 4 ulp (fp32) of the reference value; the five counts exactly;
  * coef: 1 ulp (fp32) of the reference (one rounding of an fp64 expression);
  * mel gradient: exactly sign(pred - tgt) * coef[0], 0 where masked, filtered or tied;
  * other gradients: absolute, in units of 2^-23 * |coef_k| * m_k with m = delta (Huber terms) or max(1, pos_weight) (stop).  GRAD_UNITS
    allows each tensor 4x the largest multiple it showed on an MI355X over every case of this file:
        tensor    largest measured (case)              allowed
        duration  4.554 (one_workgroup_m1)             18.216
        stop      1.080 (above_grid_caps)               4.320
        pitch     0.344 (one_workgroup_m1)              1.376
        energy    0.344 (one_workgroup_m1)              1.376
    (per case, duration / stop / pitch / energy: existing 4.216 0.416 0.307 0.313; one_workgroup_m1 4.554 0.000 0.344 0.344; odd_ragged_m7
    4.279 0.555 0.266 0.335; above_grid_caps 4.317 1.080 0.263 0.262; non-finite elements 4.216 0.419 0 0 (coef = 2^-8: the product is
    exact); two shards 3.475 0.380 0.256 0.256.)  A multiple above 16 would be a finding, not a bound to move; none is.  The duration
    figure is the device logf: log(d + 1) lies in [4, 8) for d >= 54, where one fp32 ulp is 4 units, so a logf within 1 ulp plus half a unit
    each for the subtraction and the product gives up to 5.  The other three are the subtraction and the product alone, and for stop expf
    and the division under a weight of at most 17.

Measured on an MI355X.  Error against the reference in fp32 ulps of the reference value, for the kernel and for fp32 torch (O.losses /
O.loss_sums, the yardstick), and kernel / torch.  Columns: total, mel, duration, stop, pitch, energy loss | the five sums in that order.
    existing            kernel  0.89  0.24  0.13  0.27  0.49  0.35  |   0.00  0.31  0.00  0.23  0.17
                        torch   1.11  0.76  0.13  0.27  0.49  0.35  |   0.77  0.25  0.43  0.70  0.51
                        ratio   0.81  0.32  1.00  1.00  1.00  1.00  |   0.01  1.24  0.01  0.33  0.34
    one_workgroup_m1    kernel  0.44  0.20  0.31  0.20  0.57  0.74  |   0.00  0.01  0.00  0.17  0.18
                        torch   0.44  0.20  1.69  0.20  0.57  0.74  |   0.00  1.20  0.00  0.71  0.21
                        ratio   1.00  1.00  0.18  1.00  1.00  1.00  |      -  0.01  0.00  0.23  0.85
    odd_ragged_m7       kernel  0.23  0.17  1.83  0.30  0.42  0.13  |   0.01  1.79  0.00  0.01  0.01
                        torch   0.23  0.83  0.17  0.70  0.58  0.87  |   0.62  0.15  0.50  0.16  0.36
                        ratio   1.00  0.20 10.47  0.43  0.71  0.14  |   0.01 11.70  0.01  0.03  0.02
    above_grid_caps     kernel  0.01  0.21  0.10  0.08  0.10  0.11  |   0.00  0.23  0.00  0.01  0.03
                        torch   0.01  0.21  1.10  0.08  1.10  0.89  |   0.01  0.54  0.36  0.59  0.91
                        ratio   1.00  1.00  0.09  1.00  0.09  0.12  |   0.05  0.43  0.01  0.02  0.03
    non-finite elements kernel  0.68  0.24  0.13  0.22  0.61  0.35  |   0.01  0.31  0.02  0.23  0.17
                        torch   0.32  0.76  0.13  0.22  0.61  0.35  |   none  0.25  none  none  none
                        ratio   2.09  0.32  1.00  1.00  1.00  1.00  |   none  1.24  none  none  none
    two shards          kernel  0.90  0.44  1.65  0.16  0.27  0.22  |   0.00  1.30  0.00  0.02  0.03
                        torch   0.90  0.56  0.35  0.84  0.27  0.22  |   0.34  0.81  0.68  0.12  0.36
                        ratio   1.00  0.78  4.64  0.19  1.00  1.00  |   0.01  1.60  0.00  0.18  0.09
  "none": O.loss_sums has no finite filter, so that sum has no yardstick and the kernel is held to the 4-ulp floor alone.  Where the ratio is
  above 4 (odd_ragged_m7 duration loss and sum, two shards duration loss) the yardstick happens to be nearly exact and the floor decides:
  the largest such kernel error is 1.83 ulp against the floor of 4.  Every other case of the file repeats the figures of "existing" on
  the terms it leaves alone.  coef: at most 0.49 ulp over all 155 coefficients compared (bound 1 ulp).  test_adaptive_scale: every loss within
  half an ulp (one rounding of the fp64 mean).  Counts, mel gradients, kk_frame_mask and kk_pad2d_f32: exact.
"""
import math

import numpy as np
import pytest
import torch

from oracle import kokoro_oracle as O

gpu = pytest.mark.gpu

HP = O.StepHyper()
LOSS_SCALE = 0.5
CAPS = (100.0, 100.0, 100.0, 10.0, 10.0)
TERMS = ("mel", "dur", "stop", "pitch", "energy")
PRED = ("mel", "dur_p", "stop", "pitch", "energy")


def f32(v):
    """The value the kernels see: the configuration struct carries floats."""
    return float(np.float32(v))


W = (1.0, f32(HP.duration_loss_weight), f32(HP.stop_token_loss_weight), f32(HP.pitch_loss_weight), f32(HP.energy_loss_weight))
D_DUR, D_PITCH, D_ENERGY = f32(HP.duration_huber_delta), f32(HP.pitch_huber_delta), f32(HP.energy_huber_delta)
PW = f32(HP.stop_token_pos_weight)
MAG = {"dur": D_DUR, "stop": max(1.0, PW), "pitch": D_PITCH, "energy": D_ENERGY}
# allowed multiple of 2^-23 * |coef| * MAG per gradient tensor: 4x the largest measured on an MI355X (module docstring)
GRAD_UNITS = {"dur": 4 * 4.554, "stop": 4 * 1.080, "pitch": 4 * 0.344, "energy": 4 * 0.344}


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


# ------------------------------------------------------------------------------------------------------------ the fp64 reference
def _huber(e, delta):
    a = e.abs()
    return torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))


def _logsig(z):
    return torch.clamp(z, max=0.0) - torch.log1p(torch.exp(-z.abs()))


def _masks(x):
    T, P = x["mel"].shape[1], x["dur"].shape[1]
    fm = torch.arange(T)[None, :] < x["mel_len"][:, None]
    pm = torch.arange(P)[None, :] < x["ph_len"][:, None]
    return fm, pm


def ref_terms(x, pred=None):
    """[(per-element term, kept-element mask)] in the order mel, dur, stop, pitch, energy; everything fp64."""
    p = pred if pred is not None else {k: x[k].double() for k in PRED}
    fm, pm = _masks(x)
    l1 = (p["mel"] - x["mel_t"].double()).abs()
    ld = _huber(p["dur_p"] - torch.log(x["dur"].double() + 1.0), D_DUR)
    z, y = p["stop"], x["stop_t"].double()
    ls = -(PW * y * _logsig(z) + (1.0 - y) * _logsig(-z))
    lp = _huber(p["pitch"] - x["pitch_t"].double(), D_PITCH)
    le = _huber(p["energy"] - x["energy_t"].double(), D_ENERGY)
    return [(l1, fm[..., None] & torch.isfinite(l1)), (ld, pm & (x["dur"] > 0)), (ls, fm & torch.isfinite(ls)),
            (lp, fm & torch.isfinite(lp)), (le, fm & torch.isfinite(le))]


def ref_scale(T, max_dur, adaptive):
    scale = f32(LOSS_SCALE)
    if adaptive:
        risk = max(T / 1400.0, max_dur / 150.0 if max_dur is not None else 0.0)
        if risk > 1.0:
            scale *= max(0.25, 1.0 / risk)
    return scale


def ref_finalize(sums, counts, T, max_dur=None, adaptive=0):
    """(losses[6], coef[5]) from fp64 sums and integer counts."""
    scale = ref_scale(T, max_dur, adaptive)
    vals, coef = [], []
    for s, c, cap, w in zip(sums, counts, CAPS, W):
        mean = s / c if c > 0 else 0.0
        is_open = c > 0 and mean <= cap                  # clamp(max=cap) passes no gradient above the cap; NaN is never open
        vals.append(cap if mean > cap else mean)
        coef.append(w * scale / c if is_open else 0.0)
    return np.array([sum(v * w for v, w in zip(vals, W))] + vals), np.array(coef)


def ref_unit_grads(x):
    """d(sum of the kept terms) / d(prediction) in closed form: the gradient tensors are coef[k] times these."""
    terms = ref_terms(x)
    zero = lambda t: torch.zeros_like(t)
    e = x["mel"].double() - x["mel_t"].double()
    g_mel = torch.where(terms[0][1], torch.sign(e), zero(e))
    e = x["dur_p"].double() - torch.log(x["dur"].double() + 1.0)
    g_dur = torch.where(terms[1][1], e.clamp(-D_DUR, D_DUR), zero(e))
    z, y = x["stop"].double(), x["stop_t"].double()
    g_stop = torch.where(terms[2][1], (1.0 - y) * torch.sigmoid(z) - PW * y * torch.sigmoid(-z), zero(z))
    e = x["pitch"].double() - x["pitch_t"].double()
    g_pitch = torch.where(terms[3][1], e.clamp(-D_PITCH, D_PITCH), zero(e))
    e = x["energy"].double() - x["energy_t"].double()
    g_energy = torch.where(terms[4][1], e.clamp(-D_ENERGY, D_ENERGY), zero(e))
    return [g_mel, g_dur, g_stop, g_pitch, g_energy]


def ref_all(x, T=None, max_dur=None, adaptive=0):
    terms = ref_terms(x)
    sums = [float(v[m].sum()) for v, m in terms]
    counts = [int(m.sum()) for _, m in terms]
    losses, coef = ref_finalize(sums, counts, T if T is not None else x["mel"].shape[1], max_dur, adaptive)
    return dict(sums=sums, counts=counts, losses=losses, coef=coef, unit=ref_unit_grads(x))


# ------------------------------------------------------------------------------------------------------------ inputs
OFF_DUR = (-2.5, -1.0, -0.3, 0.0, 0.4, 1.0, 1.7)            # both sides of delta = 1.0 and exactly at +-delta
OFF_VAR = (-0.2, -0.05, -0.02, 0.0, 0.03, 0.05, 0.3)        # the same for delta = 0.05
# (logit, target kind: 0 / 1 / soft 0.25), planted at frame index i % STOP_PERIOD == j of the flattened (B, T) grid.  A wrong-side
# saturated logit costs up to 100 (1700 with pos_weight), so the period spreads the eighteen over enough ordinary frames to keep the mean
# below its cap of 100.  The smallest table shape, (2, 3, 700, 1), has six frames, five of them valid, and receives the first six entries
# only: the one wrong-side term there is (88, soft 0.25) = 0.75 * 88 = 66, a mean of about 13.  test_losses_against_fp64 asserts the mean.
STOP_PLANT = [(30.0, 1), (-30.0, 0), (88.0, 2), (-88.0, 0), (100.0, 1), (-100.0, 0),
              (30.0, 0), (-30.0, 1), (88.0, 0), (-88.0, 1), (100.0, 0), (-100.0, 1),
              (30.0, 2), (-30.0, 2), (88.0, 1), (-88.0, 2), (100.0, 2), (-100.0, 2)]
STOP_PERIOD = 131                                            # keeps the planted BCE values (up to 1700) from lifting the mean above its cap


def make_inputs(B, T, P, M, mel_len, ph_len, seed, plant):
    g = torch.Generator().manual_seed(seed)
    mel_len, ph_len = torch.tensor(mel_len, dtype=torch.long), torch.tensor(ph_len, dtype=torch.long)
    assert mel_len.shape == (B,) and ph_len.shape == (B,) and int(mel_len.max()) <= T and int(ph_len.max()) <= P
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    # padded frames and positions hold ordinary values in predictions AND targets: only the masks keep them out
    mel_t = (rn(B, T, M) * 2 - 5).clamp(-11.5, 2.0)
    mel = mel_t + rn(B, T, M)
    dur = torch.randint(1, 60, (B, P), generator=g)
    dur_p = torch.log(dur.float() + 1.0) + rn(B, P) * 0.8
    stop = rn(B, T) * 3
    stop_t = torch.zeros(B, T)
    for b in range(B):                                       # the data set's smoothed tail: ... 1/8 1/4 1/2 1
        t = int(mel_len[b])
        n = min(7, t)
        if n:
            stop_t[b, t - n:t] = (0.5 ** torch.arange(n, dtype=torch.float32)).flip(0)
    pitch_t = ru(B, T)
    pitch_t[ru(B, T) < 0.3] = 0.0
    pitch = pitch_t + rn(B, T) * 0.06
    energy_t = ru(B, T)
    energy = energy_t + rn(B, T) * 0.06
    if plant:
        tie = ru(B, T, M) < 0.05
        mel[tie] = mel_t[tie]                                # exact ties: gradient 0
        k = torch.arange(B * P).view(B, P) % 17
        dur[(k == 7) | (k == 12)] = 0                        # d == 0 inside ph_len: excluded and not counted
        for j, off in enumerate(OFF_DUR):
            dur_p[k == j] = torch.log(dur[k == j].float() + 1.0) + off
        beyond = torch.arange(P)[None, :] >= ph_len[:, None]
        dur[beyond] = dur[beyond].clamp(min=3)               # d > 0 beyond ph_len: excluded by position
        i = torch.arange(B * T).view(B, T)
        for tgt, prd, shift in ((pitch_t, pitch, 0), (energy_t, energy, 3)):
            k = (i + shift) % 11
            for j, off in enumerate(OFF_VAR):
                sel = k == j
                tgt[sel & ((i // 11) % 2 == 0)] = 0.0        # target 0: the error is the offset exactly (|e| == delta where it is +-0.05)
                prd[sel] = tgt[sel] + off
        soft = ru(B, T) < 0.2
        stop_t[soft] = ru(B, T)[soft].clamp(0.01, 0.99)
        k = i % STOP_PERIOD
        for j, (zv, kind) in enumerate(STOP_PLANT):
            stop[k == j] = zv
            stop_t[k == j] = (0.0, 1.0, 0.25)[kind]
    return dict(mel=mel, mel_t=mel_t, dur_p=dur_p, dur=dur, stop=stop, stop_t=stop_t, pitch=pitch, pitch_t=pitch_t, energy=energy,
                energy_t=energy_t, mel_len=mel_len, ph_len=ph_len)


SHAPES = {
    "existing": dict(B=3, T=50, P=9, M=80, mel_len=[50, 37, 44], ph_len=[9, 6, 8], seed=11, plant=False),
    "one_workgroup_m1": dict(B=2, T=3, P=700, M=1, mel_len=[3, 2], ph_len=[700, 433], seed=12, plant=True),
    "odd_ragged_m7": dict(B=5, T=77, P=13, M=7, mel_len=[77, 0, 41, 5, 63], ph_len=[13, 7, 0, 1, 10], seed=13, plant=True),
    "above_grid_caps": dict(B=16, T=1650, P=40, M=80, seed=14, plant=True,
                            mel_len=[1650, 1649, 1401, 1237, 1024, 1000, 777, 513, 512, 300, 129, 64, 33, 7, 3, 1400],
                            ph_len=[40, 39, 33, 32, 31, 27, 25, 17, 16, 12, 9, 8, 5, 2, 1, 40]),
}


def base_inputs():
    return make_inputs(**SHAPES["existing"])


def clone(x):
    return {k: v.clone() for k, v in x.items()}


def shard(x, lo, hi):
    return {k: v[lo:hi].clone() for k, v in x.items()}


def to_oracle(x):
    out = {"mel": x["mel"], "log_dur": x["dur_p"], "stop": x["stop"], "pitch": x["pitch"], "energy": x["energy"]}
    batch = {"mel_specs": x["mel_t"], "phoneme_durations": x["dur"], "stop_token_targets": x["stop_t"], "pitches": x["pitch_t"],
             "energies": x["energy_t"], "mel_lengths": x["mel_len"], "phoneme_lengths": x["ph_len"]}
    return out, batch


def yardstick(xs):
    """fp32 torch on the same inputs (a list of shards, reduced like a data-parallel run): (losses[6], sums[5]) as floats.
    O.loss_sums has no finite filter, so a sum that holds a non-finite element comes back non-finite: check_scalar then has no yardstick
    for it and holds the kernel to the 4-ulp floor alone."""
    sums, counts = None, None
    for x in xs:
        s, c = O.loss_sums(*to_oracle(x), HP)
        sums = s if sums is None else [a + b for a, b in zip(sums, s)]
        counts = c if counts is None else [a + b for a, b in zip(counts, c)]
    if len(xs) == 1:
        ls = O.losses(*to_oracle(xs[0]), HP)
    else:
        ls = O.losses_from_sums(sums, counts, HP)
    return [float(v) for v in ls], [float(v) for v in sums]


# ------------------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_self_check():
    """The closed-form gradients equal fp64 autograd of the reference's own forward (planted input, adaptive scale, one clamped and one
    empty term), and the forward equals O.losses on a synthetic batch to fp32 accuracy.

    The fp32 bound: every element of a term costs a handful of fp32 roundings of O(1) operands (|log(d + 1)| <= 7, one rounding and one
    libm error of at most 1 ulp each: <= 5e-7 absolute on a Huber error whose slope is <= 1, against term means of 0.3 and more), and the
    pairwise fp32 sum adds log2(n) half-ulps: 16 ulp of the value covers the worst element; the averages lie far below it."""
    x = make_inputs(**SHAPES["odd_ragged_m7"])
    x["energy"] += 400.0                                     # energy mean above its cap: coefficient 0
    x["ph_len"][:] = 0                                       # the duration term empty: coefficient 0
    T, max_dur = 2000, 300
    pred = {k: x[k].double().requires_grad_(True) for k in PRED}
    terms = ref_terms(x, pred)
    sums = [v[m].sum() for v, m in terms]
    counts = [int(m.sum()) for _, m in terms]
    losses, coef = ref_finalize([float(s.detach()) for s in sums], counts, T, max_dur, 1)
    scale = ref_scale(T, max_dur, 1)
    assert scale == f32(LOSS_SCALE) * 0.5 and counts[1] == 0 and losses[5] == 10.0 and coef[1] == 0.0 and coef[4] == 0.0
    assert all(coef[k] > 0 for k in (0, 2, 3))
    objective = sum(torch.clamp(s / c, max=cap) * w for s, c, cap, w in zip(sums, counts, CAPS, W) if c > 0) * scale
    objective.backward()
    for k, (name, gu) in enumerate(zip(PRED, ref_unit_grads(x))):
        auto = pred[name].grad if pred[name].grad is not None else torch.zeros_like(gu)     # (the empty term is not in the objective)
        closed = coef[k] * gu
        err = float((auto - closed).abs().max())
        assert err <= 1e-12 * max(float(closed.abs().max()), 1e-300), (name, err)
        assert coef[k] == 0.0 or float(closed.abs().max()) > 0

    d = O.ModelDims()
    b = O.synthetic_batch(3, 50, 9, d, seed=5, ragged=True)
    g = torch.Generator().manual_seed(1)
    x = dict(mel=torch.randn(3, 50, 80, generator=g) - 5, dur_p=torch.randn(3, 9, generator=g) + 1.5, stop=torch.randn(3, 50, generator=g) * 3,
             pitch=torch.rand(3, 50, generator=g), energy=torch.rand(3, 50, generator=g), mel_t=b["mel_specs"], dur=b["phoneme_durations"],
             stop_t=b["stop_token_targets"], pitch_t=b["pitches"], energy_t=b["energies"], mel_len=b["mel_lengths"], ph_len=b["phoneme_lengths"])
    x["mel"][0, 3, 4] = float("nan")
    ref = ref_all(x)
    ls, sums32 = yardstick([x])
    for k in range(6):
        assert abs(ls[k] - ref["losses"][k]) <= 16 * ulp32(ref["losses"][k]), (k, ls[k], ref["losses"][k])
    s, c = O.loss_sums(*to_oracle(x), HP)
    assert [int(v) for v in c][1:] == ref["counts"][1:]      # (O.loss_sums counts the NaN mel element; O.losses drops it)
    assert int(c[0]) == ref["counts"][0] + 1


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def cfg_of(adaptive=0):
    from kokoro_ruslan_amd.lib import KkLossCfg
    return KkLossCfg(HP.duration_loss_weight, HP.stop_token_loss_weight, HP.pitch_loss_weight, HP.energy_loss_weight,
                     HP.duration_huber_delta, HP.pitch_huber_delta, HP.energy_huber_delta, HP.stop_token_pos_weight, LOSS_SCALE, adaptive)


def dev(x):
    return {k: v.cuda().contiguous() for k, v in x.items()}


def largs(xd, cfg):
    B, T, M = xd["mel"].shape
    return (xd["mel"], xd["mel_t"], xd["dur_p"], xd["dur"], xd["stop"], xd["stop_t"], xd["pitch"], xd["pitch_t"], xd["energy"],
            xd["energy_t"], xd["mel_len"], xd["ph_len"], B, T, xd["dur"].shape[1], M, cfg)


def new_acc():
    return torch.full((12,), 7.0, dtype=torch.float64, device="cuda")        # flags = 0 must zero-fill it


def fwd(kk, xd, adaptive=0, max_dur=None, guard=None, flags=0, acc=None):
    acc = new_acc() if acc is None else acc
    losses, coef = torch.full((6,), -3.0, device="cuda"), torch.full((5,), -3.0, device="cuda")
    md = torch.tensor([max_dur], dtype=torch.long, device="cuda") if max_dur is not None else None
    kk.call("kk_losses_fwd", *largs(xd, cfg_of(adaptive)), md, acc, losses, coef, guard, flags)
    return losses, coef, acc


def bwd(kk, xd, coef):
    grads = [torch.full_like(xd[k], float("nan")) for k in PRED]             # every element must be written
    kk.call("kk_losses_bwd", *largs(xd, cfg_of()), coef, *grads)
    return grads


def check_scalar(what, got, ref, yard):
    if math.isnan(ref):
        assert math.isnan(got), (what, got)
        return
    err = abs(got - ref)
    yerr = abs(yard - ref) if yard is not None and math.isfinite(yard) else 0.0
    floor = 4 * ulp32(ref)
    ratio = err / yerr if yerr > 0 else float("inf") if err > 0 else 0.0
    print(f"  {what}: ref {ref:.9g} kernel err {err:.3e} fp32 torch err {yerr:.3e} ratio {ratio:.2f} err/ulp32 {err / ulp32(ref):.2f}")
    assert math.isfinite(got) and err <= max(4 * yerr, floor), (what, got, ref, err, yerr, floor)


def check_coef(what, coef, ref_coef):
    got = coef.double().cpu().numpy()
    for k in range(5):
        err = abs(got[k] - ref_coef[k])
        print(f"  {what} coef[{k}]: ref {ref_coef[k]:.9g} err/ulp32 {err / ulp32(ref_coef[k]) if ref_coef[k] else err:.2f}")
        if ref_coef[k] == 0.0:
            assert got[k] == 0.0, (what, k, got[k])
        else:
            assert err <= ulp32(ref_coef[k]), (what, k, got[k], ref_coef[k])


def check_fwd(what, got, ref, yard, check_acc=True):
    losses, coef, acc = got
    ls, sums32 = yard
    lv = losses.double().cpu().numpy()
    for k in range(6):
        check_scalar(f"{what} losses[{k}]", float(lv[k]), float(ref["losses"][k]), ls[k])
    check_coef(what, coef, ref["coef"])
    if check_acc:
        a = acc.cpu().numpy()
        assert [float(v) for v in a[5:10]] == [float(c) for c in ref["counts"]], (what, a[5:10], ref["counts"])
        for k in range(5):
            check_scalar(f"{what} acc[{k}] ({TERMS[k]} sum)", float(a[k]), ref["sums"][k], sums32[k])
        assert a[11] == 0.0


def check_grads(what, grads, coef, unit):
    """`coef`: what the backward was given (the forward's own output, already held to 1 ulp of the reference)."""
    c = coef.double().cpu().numpy()
    worst = {}
    for k, (name, g, gu) in enumerate(zip(TERMS, grads, unit)):
        g = g.cpu()
        assert bool(torch.isfinite(g).all()), (what, name)
        if c[k] == 0.0:
            assert float(g.abs().max()) == 0.0, (what, name)
            continue
        if k == 0:
            assert torch.equal(g, (gu * c[0]).float()), (what, "mel gradient is not +-coef[0] / 0")
            continue
        assert bool((g[gu == 0] == 0).all()), (what, name, "non-zero gradient on an excluded element")
        mult = float((g.double() - c[k] * gu).abs().max()) / (2.0 ** -23 * abs(c[k]) * MAG[name])
        worst[name] = mult
        print(f"  {what} d{name}: max error {mult:.3f} units of 2^-23 * coef * {MAG[name]:g} (allowed {GRAD_UNITS[name]:.3f})")
        assert mult <= GRAD_UNITS[name], (what, name, mult)
    return worst


def run_case(kk, what, x, adaptive=0, max_dur=None, T=None):
    print(f"{what}:")
    xd = dev(x)
    ref = ref_all(x, T, max_dur, adaptive)
    got = fwd(kk, xd, adaptive, max_dur)
    check_fwd(what, got, ref, yardstick([x]))
    assert float(got[2][10]) == 0.0 or not all(bool(torch.isfinite(x[k]).all()) for k in PRED)
    grads = bwd(kk, xd, got[1])
    check_grads(what, grads, got[1], ref["unit"])
    return ref, got, grads


# ------------------------------------------------------------------------------------------------------------ GPU: the loss kernels
@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_losses_against_fp64(kk, name):
    s = SHAPES[name]
    x = make_inputs(**s)
    adaptive = 1 if s["T"] > 1400 else 0
    max_dur = int(x["dur"].max()) if adaptive else None
    ref, got, grads = run_case(kk, name, x, adaptive, max_dur)
    # properties of the planted input, not of the kernel: every term open, and the stop mean clear of its cap in spite of the saturated logits
    assert all(c > 0 for c in ref["coef"]), "the case must leave every term open"
    assert ref["losses"][3] < 0.5 * CAPS[2], ("planted stop logits lift the BCE mean too close to its cap", ref["losses"][3])
    if s["plant"]:
        fm, pm = _masks(x)
        assert ref["counts"][1] == int((pm & (x["dur"] > 0)).sum()) < int(pm.sum())     # zero durations inside ph_len went uncounted
        assert int(((x["dur"] > 0) & ~pm).sum()) > 0
    if adaptive:
        assert ref_scale(s["T"], max_dur, 1) < f32(LOSS_SCALE)


@gpu
def test_clamped_means(kk):
    """Above its cap a mean is held at the cap and passes no gradient: coef 0 and an all-zero gradient tensor; the other terms unchanged."""
    x = base_inputs()
    _, base, _ = run_case(kk, "unclamped", x)
    x["mel"] += 150.0
    x["pitch"] += 400.0                                      # Huber(0.05) of 400: 20 > 10
    ref, got, grads = run_case(kk, "clamped", x)
    losses, coef = got[0].cpu(), got[1].cpu()
    assert float(losses[1]) == 100.0 and float(losses[4]) == 10.0
    assert float(coef[0]) == 0.0 and float(coef[3]) == 0.0
    assert torch.equal(coef[[1, 2, 4]], base[1].cpu()[[1, 2, 4]]) and bool((coef[[1, 2, 4]] > 0).all())
    assert float(grads[0].abs().max()) == 0.0 and float(grads[3].abs().max()) == 0.0
    assert all(float(grads[k].abs().max()) > 0 for k in (1, 2, 4))


@gpu
@pytest.mark.parametrize("empty", ["frames", "phonemes"])
def test_empty_terms(kk, empty):
    x = base_inputs()
    x["mel_len" if empty == "frames" else "ph_len"][:] = 0
    ref, got, grads = run_case(kk, f"no valid {empty}", x)
    losses, coef, acc = (t.cpu() for t in got)
    gone = (0, 2, 3, 4) if empty == "frames" else (1,)
    for k in range(5):
        if k in gone:
            assert float(losses[1 + k]) == 0.0 and float(coef[k]) == 0.0 and float(acc[k]) == 0.0 and float(acc[5 + k]) == 0.0
            assert float(grads[k].abs().max()) == 0.0
        else:
            assert float(coef[k]) > 0 and float(grads[k].abs().max()) > 0
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(coef).all()) and bool(torch.isfinite(acc).all())


@gpu
def test_adaptive_scale(kk):
    """kk_losses_finalize on a fixed accumulator: the scale multiplies coef only, follows the larger of the two risks, is floored at 0.25
    and stays off without `adaptive`."""
    sums, counts = [12345.5, 7.25, 88.0, 0.9, 1.1], [4000, 20, 50, 50, 50]
    cases = [(1, T, None) for T in (1400, 1401, 2800, 5600, 9000)] + [(1, 50, m) for m in (150, 151, 300, 1000)]
    cases += [(1, 2800, 151), (1, 1401, 450), (1, 9000, 1000), (1, 50, None), (0, 9000, 1000), (0, 9000, None)]
    first = None
    seen = set()
    for adaptive, T, max_dur in cases:
        acc = torch.tensor(sums + [float(c) for c in counts] + [0.0, 0.0], dtype=torch.float64, device="cuda")
        before = acc.clone()
        losses, coef = torch.full((6,), -3.0, device="cuda"), torch.full((5,), -3.0, device="cuda")
        md = torch.tensor([max_dur], dtype=torch.long, device="cuda") if max_dur is not None else None
        kk.call("kk_losses_finalize", acc, cfg_of(adaptive), md, T, losses, coef, None, 0)
        ref_l, ref_c = ref_finalize(sums, counts, T, max_dur, adaptive)
        what = f"adaptive={adaptive} T={T} max_dur={max_dur}"
        print(f"{what}: scale {ref_scale(T, max_dur, adaptive):.6f}")
        check_coef(what, coef, ref_c)
        for k in range(6):
            check_scalar(f"{what} losses[{k}]", float(losses[k]), float(ref_l[k]), None)
        first = losses.clone() if first is None else first
        assert torch.equal(losses, first), "the losses must not change with the scale"
        assert torch.equal(acc, before)                      # clear = 0
        seen.add(round(ref_scale(T, max_dur, adaptive) / f32(LOSS_SCALE), 6))
    assert seen == {1.0, round(1400 / 1401, 6), 0.5, 0.25, round(150 / 151, 6), round(1 / 3, 6)}


def _assert_vetoed(kk, xd, got, guard, flagged_calls):
    losses, coef, acc = got
    assert float(coef.abs().max()) == 0.0
    assert guard.cpu().tolist() == [1.0, float(flagged_calls)]
    for g in bwd(kk, xd, coef):
        assert float(g.abs().max()) == 0.0                   # (also: no NaN sentinel left, none made from 0 * NaN)


@gpu
def test_guard_nonfinite_output_in_padding(kk):
    """A NaN prediction in a padded frame changes no loss, but with a guard slot it vetoes the micro-batch: coef 0, guard[0] = 1,
    guard[1] counts the flagged calls.  Without a guard slot the call is the loss function alone: no veto."""
    x = base_inputs()
    assert int(x["mel_len"][1]) < 50
    x["mel"][1, 49, 5] = float("nan")
    xd = dev(x)
    ref, yard = ref_all(x), yardstick([x])
    guard = torch.zeros(2, dtype=torch.float64, device="cuda")
    for call in (1, 2):
        got = fwd(kk, xd, guard=guard)
        vetoed = dict(ref, coef=np.zeros(5))
        check_fwd(f"guarded call {call}", got, vetoed, yard)
        assert float(got[2][10]) > 0
        _assert_vetoed(kk, xd, got, guard, call)
    run_case(kk, "same input, no guard slot", x)
    assert guard.cpu().tolist() == [1.0, 2.0]


@gpu
def test_guard_nonfinite_duration_loss(kk):
    """The duration term has no finite filter: a NaN dur_pred in a counted position makes that loss and the total NaN, its coefficient 0
    (a NaN mean is not below the cap) and, with a guard slot, flags the micro-batch."""
    x = base_inputs()
    assert int(x["dur"][0, 2]) > 0 and int(x["ph_len"][0]) > 2
    x["dur_p"][0, 2] = float("nan")
    xd = dev(x)
    ref = ref_all(x)
    assert math.isnan(ref["losses"][0]) and math.isnan(ref["losses"][2]) and ref["coef"][1] == 0.0 and all(ref["coef"][k] > 0 for k in (0, 2, 3, 4))
    got = fwd(kk, xd)
    check_fwd("NaN dur_pred, no guard slot", got, ref, yardstick([x]))
    grads = bwd(kk, xd, got[1])
    check_grads("NaN dur_pred, no guard slot", grads, got[1], ref["unit"])
    guard = torch.zeros(2, dtype=torch.float64, device="cuda")
    got = fwd(kk, xd, guard=guard)
    check_fwd("NaN dur_pred, guarded", got, dict(ref, coef=np.zeros(5)), yardstick([x]))
    _assert_vetoed(kk, xd, got, guard, 1)


@gpu
def test_guard_untouched_by_a_clean_batch(kk):
    x = base_inputs()
    guard = torch.tensor([0.0, 3.0], dtype=torch.float64, device="cuda")
    got = fwd(kk, dev(x), guard=guard)
    check_fwd("clean batch, guarded", got, ref_all(x), yardstick([x]))
    assert guard.cpu().tolist() == [0.0, 3.0] and float(got[2][10]) == 0.0


@gpu
def test_nonfinite_elements_are_dropped(kk):
    """inf / NaN in valid positions of the filtered terms, in predictions and in targets: out of the sum and of the count, gradient 0."""
    x = base_inputs()
    base = ref_all(x)
    nan, inf = float("nan"), float("inf")
    plant = {"mel": [((0, 3, 4), nan), ((0, 5, 7), inf), ((2, 0, 0), -inf)], "mel_t": [((0, 6, 1), inf), ((1, 2, 3), nan)],
             "stop": [((0, 4), inf), ((1, 1), nan)], "stop_t": [((0, 7), nan)],
             "pitch": [((0, 2), nan), ((2, 3), -inf)], "pitch_t": [((1, 5), inf)],
             "energy": [((0, 9), inf), ((1, 0), nan)], "energy_t": [((2, 2), nan)]}
    for key, items in plant.items():
        for idx, v in items:
            assert idx[1] < int(x["mel_len"][idx[0]])
            x[key][idx] = v
    ref, got, grads = run_case(kk, "non-finite elements", x)
    assert [b - c for b, c in zip(base["counts"], ref["counts"])] == [5, 0, 3, 3, 3]
    assert [float(v) for v in got[2][5:10].cpu()] == [float(c) for c in ref["counts"]]
    for key, items in plant.items():
        k = PRED.index(key[:-2] if key.endswith("_t") else key)
        for idx, _ in items:
            assert float(grads[k][idx]) == 0.0, (key, idx)
    assert float(got[2][10]) > 0                              # the finite-output guard saw them (no guard slot: no veto)


@gpu
def test_two_shards_one_accumulator(kk):
    """The data-parallel order: both shards add into one accumulator, kk_losses_finalize normalises by the counts of the whole batch."""
    x = make_inputs(B=6, T=50, P=9, M=80, mel_len=[50, 31, 44, 9, 50, 27], ph_len=[9, 5, 8, 2, 9, 6], seed=21, plant=True)
    parts = [shard(x, 0, 2), shard(x, 2, 6)]
    pd = [dev(p) for p in parts]
    ref = ref_all(x)
    acc = new_acc()
    fwd(kk, pd[0], flags=0, acc=acc)
    fwd(kk, pd[1], flags=1, acc=acc)                          # KK_LOSS_ACC_ZEROED: no zero-fill, adds to the first shard's sums
    losses, coef = torch.full((6,), -3.0, device="cuda"), torch.full((5,), -3.0, device="cuda")
    summed = acc.clone()
    kk.call("kk_losses_finalize", acc, cfg_of(), None, 50, losses, coef, None, 1)
    print("two shards:")
    check_fwd("two shards", (losses, coef, summed), ref, yardstick(parts))
    assert all(c > 0 for c in ref["coef"])
    assert float(acc.abs().max()) == 0.0                      # clear = 1
    grads = [torch.cat(g) for g in zip(*(bwd(kk, p, coef) for p in pd))]
    check_grads("two shards", grads, coef, ref["unit"])
    one = [float(c) for c in ref_all(parts[0])["coef"]]
    assert all(abs(a - b) > 4 * ulp32(b) for a, b in zip(one, ref["coef"]))      # (a shard's own counts would give other coefficients)


# ------------------------------------------------------------------------------------------------------------ GPU: kk_frame_mask, kk_pad2d_f32
@gpu
@pytest.mark.parametrize("B,T", [(1, 1), (3, 77), (7, 4099)])
def test_frame_mask(kk, B, T):
    values = [0, 1, T - 1, T, T + 3]
    for r in range(-(-len(values) // B)):
        lens = torch.tensor([values[(r * B + i) % len(values)] for i in range(B)], dtype=torch.long)
        mask = torch.full((B, T), 0xAB, dtype=torch.uint8, device="cuda")
        kk.call("kk_frame_mask", lens.cuda(), mask, B, T)
        want = (torch.arange(T)[None, :] >= lens[:, None]).to(torch.uint8)
        assert torch.equal(mask.cpu(), want), (B, T, lens.tolist())


# kk_elem.hip grid_for: at most 1024 workgroups of 256 threads in the product library, so 262 144 elements per pass: 1025 rows of 256 is the
# first row count past it.  A tools build can move that cap from the environment, up to grid_for's own argument default of 4096 workgroups
# (1 048 576 elements); 4097 rows of 256 take a second pass under every setting.
PAD_CASES = {"widen": (3, 5, 5, 9, 9), "narrow": (4, 1031, 1031, 1000, 1000), "equal": (5, 33, 33, 33, 33),
             "widen_ld": (3, 5, 8, 9, 12), "narrow_ld": (4, 31, 40, 20, 27), "equal_ld": (2, 6, 7, 6, 9),
             "second_pass": (1025, 250, 250, 256, 256), "one_pass_full": (1024, 250, 250, 256, 256),
             "second_pass_any_cap": (4097, 250, 250, 256, 256)}


@gpu
@pytest.mark.parametrize("case", list(PAD_CASES))
def test_pad2d(kk, case):
    rows, cols_src, lds, cols_dst, ldd = PAD_CASES[case]
    g = torch.Generator().manual_seed(rows + cols_src)
    src = torch.randn(rows, lds, generator=g) + 3.0          # (no zero in the source: a zero in the output is the kernel's)
    dst = torch.full((rows, ldd), -7.5, device="cuda")
    kk.call("kk_pad2d_f32", src.cuda(), lds, cols_src, dst, ldd, cols_dst, rows)
    want = torch.full((rows, ldd), -7.5)
    want[:, :cols_dst] = 0.0
    n = min(cols_src, cols_dst)
    want[:, :n] = src[:, :n]
    assert torch.equal(dst.cpu(), want), case
