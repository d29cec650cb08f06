"""Shared by the kernel-level fp64 suites (test_norm_kernels_gpu.py, test_tail_kernels_gpu.py): guarded device buffers, the error
measure and the bound.  Not a test.

The bound is not a fixed number: E_ref = max|fp32 PyTorch restatement - fp64| / max|fp64| on the same inputs, and the kernel's error,
normalised the same way, must be <= 4 E_ref + 2^-22 (4x: another summation tree; 2^-22: the floor where the restatement happens to be
exact); an output stored as bf16 gets one more bf16 rounding, 2^-8."""
import math

import torch

FLT_EPS = torch.finfo(torch.float32).eps
FLOOR = 2.0 ** -22
BF16_ROUND = 2.0 ** -8
SENT = -1024.0               # guard value (exact in bf16 too); no kernel output of these tests equals it by construction of the guards
NAN = float("nan")


class Guarded:
    """A [rows, cols] device view (row stride ld >= cols) inside a buffer of guard rows / columns that hold SENT."""

    def __init__(self, rows, cols, dtype=torch.float32, fill=NAN, ld=None, pad=4):
        self.rows, self.cols, self.pad = rows, cols, pad
        self.ld = ld or cols
        self.buf = torch.full((rows + 2 * pad, self.ld), SENT, dtype=dtype, device="cuda")
        self.t = self.buf[pad:pad + rows, :cols]
        if torch.is_tensor(fill):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)

    def intact(self):
        b = self.buf.clone()
        b[self.pad:self.pad + self.rows, :self.cols] = SENT
        return bool((b == SENT).all())


def gvec(n, fill):
    return Guarded(1, n, fill=fill)


def nerr(got, ref64):
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "non-finite values"
    scale, err = float(ref64.abs().max()), float((got - ref64).abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / scale


def bounded(what, got, ref32, ref64, extra=0.0, tag="fp64"):
    """kernel error <= 4 E_ref + 2^-22 (+ extra), all normalised by max|fp64|.  Returns (E_ref, kernel error)."""
    e_ref, e_k = nerr(ref32, ref64), nerr(got, ref64)
    bound = 4.0 * e_ref + FLOOR + extra
    ratio = e_k / e_ref if e_ref > 0 else (0.0 if e_k == 0 else math.inf)
    print(f"[{tag}] {what}: E_ref={e_ref:.3e} kernel={e_k:.3e} kernel/E_ref={ratio:.2f} bound={bound:.3e} "
          f"kernel/bound={e_k / bound:.2f}")
    assert e_k <= bound, f"{what}: kernel error {e_k:.3e} > 4 x {e_ref:.3e} + 2^-22{' + 2^-8' if extra else ''} = {bound:.3e}"
    return e_ref, e_k


def ln_bwd_formula(dy, x, gamma, mean, rstd):
    """LayerNorm backward from given statistics: (dx, the terms whose column sums are dgamma); dbeta is the column sum of dy."""
    xh = (x - mean[:, None]) * rstd[:, None]
    dg = dy * gamma
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    return rstd[:, None] * (dg - s1 - xh * s2), dy * xh


def rms_bwd_formula(dy, x, gain, rstd):
    """RMSNorm backward from a given 1/rms: (dx, the terms whose column sums are dgain)."""
    rs = rstd[:, None]
    dg = dy * gain
    k = (dg * x).mean(1, keepdim=True) * rs * rs * rs
    return rs * dg - x * k, dy * x * rs
