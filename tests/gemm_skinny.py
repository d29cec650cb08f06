"""Checker shared by test_gemm_skinny_gpu.py (kk_gemm at the decode step's few rows, on the device) and test_gemm_skinny_cpu.py (the
evidence that this checker accepts a correct result and rejects subtly wrong ones).  Everything here runs on the CPU: problem
construction, operand embedding, the fp64 reference, the tolerance table, the sentinel and bit checks.

A problem is C[:M, :N] = ALPHA * A.B + bias + res[row % RES_MOD] with A stored [M, K] (ta = 0) and B stored [N, K] (tb = 0, the
engine's _linear form) or [K, N] (tb = 1).  Every operand is a view, from offset 0, of a larger buffer: what lies outside the view
(pad columns up to the leading dimension, extra rows behind the last one) is filled with zeros or with NaN, so a kernel that reads
it and multiplies it by zero is told apart from one that masks it.
"""
import math

import torch

MS = (1, 2, 3, 5, 8, 16, 17, 63, 64, 65)
SHAPES = ((512, 80), (80, 512), (512, 512), (1536, 512), (512, 1536))          # (N, K): the decode step's projections
TB1_SHAPES = ((512, 512), (80, 512))
LAYOUTS = tuple((N, K, 0) for N, K in SHAPES) + tuple((N, K, 1) for N, K in TB1_SHAPES)   # (N, K, tb)
STORAGE = ((0, 0), (1, 0), (1, 2), (1, 3), (1, 7))                              # (math, dtypes): dtypes bit 0 / 1 / 2 = A / B / C held as bf16
ALPHA, RES_MOD, SENTINEL = 0.5, 5, 7.0
A_PAD_COLS, B_PAD_COLS, C_PAD_COLS, R_PAD_COLS = 16, 8, 24, 8
AB_EXTRA_ROWS, C_EXTRA_ROWS = 64, 8
R_EXTRA_ROWS = 64          # rows of the residual buffer behind the period: NaN always (a row index not taken modulo RES_MOD reads them)


def tolerance(math_mode, dtypes, K):
    """(atol, rtol) of a result against the fp64 reference: the bounds the kernel suite already uses for the same storage."""
    s = math.sqrt(K / 64)
    if math_mode == 0:
        return 2e-4 * s, 2e-5
    if dtypes in (0, 2):
        return 5e-2 * s, 1e-3
    if dtypes == 3:
        return 2e-3 * s, 1e-4
    if dtypes == 7:
        return 2e-3 * s + 0.1, 1e-2
    raise ValueError(f"no tolerance for math={math_mode} dtypes={dtypes}")


def accumulate_tolerance(K):
    """beta = 1 onto an fp32 C (the bounds of the DMA core's accumulate test)."""
    return 3e-3 * math.sqrt(K / 64), 1e-4


def _r16(t):
    return t.bfloat16().float()


class Problem:
    """One kk_gemm call: logical operands (fp32 values, bf16-representable where the storage is bf16), its buffers and reference."""

    def __init__(self, M, N, K, tb, math_mode, dtypes):
        self.M, self.N, self.K, self.tb, self.math, self.dtypes = M, N, K, tb, math_mode, dtypes
        self.a16, self.b16, self.c16 = dtypes & 1, (dtypes >> 1) & 1, (dtypes >> 2) & 1
        g = torch.Generator().manual_seed(M * 7919 + N * 31 + K * 3 + tb)     # the same operands for every storage case
        A = torch.randn(M, K, generator=g)
        B = torch.randn((K, N) if tb else (N, K), generator=g)
        self.bias = torch.randn(N, generator=g)
        self.res = torch.randn(RES_MOD, N, generator=g)
        self.acc = torch.randn(M, N, generator=g)                             # what the accumulate form adds onto
        self.res_past = torch.randn(1, N, generator=g)                        # finite stand-in for the row behind the period (wrong-period mutations)
        self.A = _r16(A) if self.a16 else A                                   # as stored
        self.B = _r16(B) if self.b16 else B
        self.lda, self.ldb = K + A_PAD_COLS, (N if tb else K) + B_PAD_COLS
        self.ldc, self.ldr = N + C_PAD_COLS, N + R_PAD_COLS
        self.c_dtype = torch.bfloat16 if self.c16 else torch.float32

    # ---- operands as the kernel's arithmetic sees them: bf16 math rounds fp32 storage when it stages it --------------------
    def seen(self):
        A, B = (_r16(self.A), _r16(self.B)) if self.math else (self.A, self.B)
        return A, (B if self.tb else B.t())                                   # [M, K], [K, N]

    def rows(self, period=RES_MOD):
        return torch.arange(self.M) % period

    def reference(self):
        """fp64: ALPHA * A.B + bias + the periodic residual."""
        if not hasattr(self, "_ref"):
            A, B = self.seen()
            self._prod = A.double() @ B.double()
            self._ref = ALPHA * self._prod + self.bias.double() + self.res.double()[self.rows()]
        return self._ref

    def accumulate_reference(self):
        """fp64: the alpha = 1, beta = 1 form without bias and residual, onto self.acc."""
        self.reference()
        return self._prod + self.acc.double()

    def fp32_result(self, A=None, B=None, bias=None, rows=None):
        """The result by plain fp32 torch (rounded to bf16 when C is stored so): what a correct device result looks like.  The
        arguments replace pieces of the computation (the CPU test's mutations)."""
        sA, sB = self.seen()
        A, B = sA if A is None else A, sB if B is None else B
        bias = self.bias if bias is None else bias
        rows = self.rows() if rows is None else rows
        return (ALPHA * (A @ B) + bias + torch.cat([self.res, self.res_past])[rows]).to(self.c_dtype)

    # ---- buffers ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _embed(x, extra_rows, ld, fill, dtype):
        buf = torch.full((x.shape[0] + extra_rows, ld), fill, dtype=dtype)
        buf[:x.shape[0], :x.shape[1]] = x.to(dtype)
        return buf

    def a_buffer(self, fill, A=None):
        return self._embed(self.A if A is None else A, AB_EXTRA_ROWS, self.lda, fill, torch.bfloat16 if self.a16 else torch.float32)

    def b_buffer(self, fill):
        return self._embed(self.B, AB_EXTRA_ROWS, self.ldb, fill, torch.bfloat16 if self.b16 else torch.float32)

    def r_buffer(self):
        buf = self._embed(self.res, R_EXTRA_ROWS, self.ldr, 0.0, torch.float32)
        buf[RES_MOD:] = math.nan
        return buf

    def c_buffer(self, result=None):
        """(M + 8) x (N + 24) of the sentinel; `result` ([M, N]) is placed in the view (the CPU test's stand-in for a launch)."""
        buf = torch.full((self.M + C_EXTRA_ROWS, self.ldc), SENTINEL, dtype=self.c_dtype)
        if result is not None:
            buf[:self.M, :self.N] = result.to(self.c_dtype)
        return buf

    def a_only_row(self, r):
        """A with every row but r set to NaN."""
        A = torch.full_like(self.A, math.nan)
        A[r] = self.A[r]
        return A

    def __repr__(self):
        return f"gemm {self.M}x{self.N}x{self.K} tb={self.tb} math={self.math} dtypes={self.dtypes}"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def check_values(got, ref, atol, rtol, what):
    """|got - ref| <= atol + rtol |ref| on every element, in fp64; a non-finite element fails."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} off; max|err|={float(err.max()):.3e} "
                                 f"max|ref|={float(ref.abs().max()):.3e} atol={atol:.3e} rtol={rtol:.1e}")


def error_ratio(got, ref, atol, rtol):
    """Largest |got - ref| / (atol + rtol |ref|): how much of the bound a result uses."""
    got, ref = got.detach().cpu().double(), ref.double()
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def check_sentinel(cbuf, M, N, what):
    """Nothing outside C[:M, :N] was written: the rest of the buffer holds the sentinel, bit for bit."""
    want = _bits(torch.full((1,), SENTINEL, dtype=cbuf.dtype))[0]
    b = _bits(cbuf)
    assert bool((b[M:] == want).all()), f"{what}: rows of the C buffer beyond M were written"
    assert bool((b[:, N:] == want).all()), f"{what}: columns of the C buffer beyond N were written"


def check_output(p, cbuf, what=""):
    """Items 1 and 2 of every case: the view against fp64 at the storage's tolerance, the rest of the buffer untouched."""
    what = what or repr(p)
    assert cbuf.dtype == p.c_dtype and tuple(cbuf.shape) == (p.M + C_EXTRA_ROWS, p.ldc), what
    check_values(cbuf[:p.M, :p.N], p.reference(), *tolerance(p.math, p.dtypes, p.K), what)
    check_sentinel(cbuf, p.M, p.N, what)


def check_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())}/{diff.numel()} elements differ in their bits"


def check_bf16_store(c16, c32, what):
    """A bf16 C is the round-to-nearest-even image of the fp32 C of the same launch, bit for bit."""
    assert c16.dtype == torch.bfloat16 and c32.dtype == torch.float32, what
    check_same_bits(c16, c32.detach().cpu().bfloat16(), f"{what}: bf16 store against the rounded fp32 store")


def truncate_bf16(c32):
    """fp32 -> bf16 by dropping the low 16 bits (the wrong conversion)."""
    return (_bits(c32) & -65536).view(torch.float32).bfloat16()
