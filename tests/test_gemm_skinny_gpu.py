"""GPU suite: kk_gemm at the row counts the decode step runs (KokoroEngine._decoder_step: M = live rows or slots, 1 .. 16 in
practice), at the real model widths, against an fp64 reference on the CPU.  M in {1, 2, 3, 5, 8, 16, 17, 63, 64, 65} (looped inside
each case), (N, K) in {(512, 80), (80, 512), (512, 512), (1536, 512), (512, 1536)}, ta = 0, tb = 0 everywhere and tb = 1 at
(512, 512) and (80, 512); fp32, bf16 math on fp32 storage, bf16 weights, bf16 operands, bf16 operands and result.  Every call is the
_stream_step form: split_k = 1, bias, a residual with a row period of 5, alpha = 0.5, beta = 0, every operand a view of a larger
buffer.  Checker, tolerances and embedding: tests/gemm_skinny.py; that they discriminate: tests/test_gemm_skinny_cpu.py.

What each case asserts, at every M: the values against fp64 at the suite's tolerance for that storage; nothing outside C[:M, :N]
written; the same bits whether the memory outside the A and B views holds zeros or NaN (over-reads are masked, not multiplied by
zero: the k tail of K = 80, the ragged row tile at every M, the ragged column tile of N = 80); row r of C unchanged when every other
row of A is NaN; beta = 0 overwrites a NaN-filled C (split_k = 1 with the bits of the first call, split_k = 0 within tolerance); a
repeated call repeats its bits; a bf16 C is the round-to-nearest-even image of the fp32 C of the same launch.  test_accumulate runs
alpha = 1, beta = 1 onto a random fp32 C with split_k in {1, 0} at M in {1, 5, 17}.

Routes (kk_last_kernel) taken on an MI355X, asserted in every case; the same at every M of the list and every (N, K) of the line:
  dtypes 3 / 7 (bf16 operands), K in {512, 1536}: the DMA core, gemm16<0,tb,64,64,3> (64x64 tiles, three stages);
  dtypes 3 / 7, K = 80 (K % 64 != 0):            the generic family, gemm<0,0,1,64,1,1>;
  dtypes 2 (bf16 weights):                        gemm<0,tb,1,64,0,1>;
  dtypes 0, math 1 / math 0:                      gemm<0,tb,1,64,0,0> / gemm<0,tb,0,64,0,0>.
No shape of the list takes gemm16_w8< or g16x<: at most 2 x 24 tiles of 64x64, and for K = 1536 the large tiles cost more bytes
through the busiest CU than the 64x64 ones.  With split_k = 0 the family stays and only the slicing and the DMA core's stage
count differ (the accumulate form with automatic k-slices ran gemm16<0,tb,64,64,2>), so those calls assert the family prefix.

Measured on an MI355X, largest share of the bound used over all M and (N, K), at K = 80 / 512 / 1536: math 0: 0.017 / 0.047 / 0.064;
math 1 dtypes 0 and 2: 5.0e-5 / 1.0e-4 / 1.9e-4; dtypes 3: 9.3e-4 / 2.0e-3 / 4.4e-3; dtypes 7: 0.23 / 0.29 / 0.32 (the bf16
rounding of the result: the figures of the plain fp32 result on the CPU); accumulate form: at most 7.9e-3.  Every bit check held,
the bf16 store against the rounded fp32 store included.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_skinny as GS  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = math.nan
IDS = [f"N{N}-K{K}-tb{tb}" for N, K, tb in GS.LAYOUTS]


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def expected_route(p):
    """kk_gemm's dispatch for these shapes: the DMA core needs both operands in bf16 and, for a k-contiguous operand, K % 64 == 0;
    fewer than 512 128x128 tiles take the generic family's 64-tile; fewer than 128 128x64 tiles take the DMA core's 64x64 tile, with
    three stages from three k-tiles per slice on."""
    if p.a16 and p.b16 and p.K % 64 == 0:
        return f"gemm16<0,{p.tb},64,64,3>"
    return f"gemm<0,{p.tb},{p.math},64,{p.a16},{p.b16}>"


def family(route):
    return route[:route.index("<") + 1]


class Launcher:
    """The device side of one Problem: kk_gemm on buffers built on the host, results returned to the host."""

    def __init__(self, kk, p):
        self.kk, self.p = kk, p
        self.bias, self.res = p.bias.cuda(), p.r_buffer().cuda()

    def stream_step(self, a_buf, b_buf, c_buf=None, ldc=None, split=1, dtypes=None, route=None):
        """alpha = 0.5, beta = 0, bias, periodic residual; C defaults to the sentinel-filled (M + 8) x (N + 24) buffer."""
        p = self.p
        dtypes = p.dtypes if dtypes is None else dtypes
        Cd = (p.c_buffer() if c_buf is None else c_buf).cuda()
        self.kk.call("kk_gemm", 0, p.tb, p.M, p.N, p.K, GS.ALPHA, a_buf, p.lda, b_buf, p.ldb, 0.0, Cd, p.ldc if ldc is None else ldc,
                     self.bias, self.res, p.ldr, GS.RES_MOD, split, p.math, dtypes)
        got, want = self.kk.last_kernel(), route or expected_route(p)
        assert got.startswith(want), (repr(p), f"split_k={split}", got, want)
        return Cd.cpu()

    def accumulate(self, a_buf, b_buf, split):
        p = self.p
        Cd = p.acc.cuda()
        self.kk.call("kk_gemm", 0, p.tb, p.M, p.N, p.K, 1.0, a_buf, p.lda, b_buf, p.ldb, 1.0, Cd, p.N, None, None, 0, 0, split, p.math,
                     p.dtypes)
        got = self.kk.last_kernel()
        assert got.startswith(expected_route(p) if split == 1 else family(expected_route(p))), (repr(p), f"split_k={split}", got)
        return Cd.cpu()


@pytest.mark.parametrize("math_mode,dtypes", GS.STORAGE, ids=[f"math{m}-dtypes{d}" for m, d in GS.STORAGE])
@pytest.mark.parametrize("N,K,tb", GS.LAYOUTS, ids=IDS)
def test_stream_step_form(kk, N, K, tb, math_mode, dtypes):
    for M in GS.MS:
        p = GS.Problem(M, N, K, tb, math_mode, dtypes)
        run = Launcher(kk, p)
        what = repr(p)
        A0, B0 = p.a_buffer(0.0).cuda(), p.b_buffer(0.0).cuda()
        # 1, 2: values against fp64, nothing outside the view written
        clean = run.stream_step(A0, B0)
        GS.check_output(p, clean, what)
        # 3: NaN instead of zeros outside the A and B views changes no bit
        masked = run.stream_step(p.a_buffer(NAN).cuda(), p.b_buffer(NAN).cuda())
        GS.check_output(p, masked, f"{what}, NaN outside the operand views")
        GS.check_same_bits(masked, clean, f"{what}: NaN against zeros outside the operand views")
        # 4: rows are independent
        for r in sorted({0, M - 1}):
            if M == 1:
                break
            alone = run.stream_step(p.a_buffer(0.0, A=p.a_only_row(r)).cuda(), B0)
            GS.check_same_bits(alone[r, :N], clean[r, :N], f"{what}: row {r} with every other row of A NaN")
            GS.check_sentinel(alone, M, N, f"{what}, NaN rows of A")
        # 6: a replayed step repeats its bits
        GS.check_same_bits(run.stream_step(A0, B0), clean, f"{what}: the same call again")
        # 5: beta = 0 overwrites (fp32 C, ldc = N, NaN before the call); the automatic split may slice K and must zero C first
        if not p.c16:
            tol = GS.tolerance(math_mode, dtypes, K)
            over = run.stream_step(A0, B0, c_buf=torch.full((M, N), NAN), ldc=N)
            GS.check_same_bits(over, clean[:M, :N].contiguous(), f"{what}: onto NaN, split_k = 1")
            auto = run.stream_step(A0, B0, c_buf=torch.full((M, N), NAN), ldc=N, split=0, route=family(expected_route(p)))
            GS.check_values(auto, p.reference(), *tol, f"{what}: onto NaN, split_k = 0")
        # 7: the bf16 store is the rounded fp32 store of the same kernel and accumulators
        if p.c16:
            p32 = GS.Problem(M, N, K, tb, math_mode, dtypes & 3)
            c32 = run.stream_step(A0, B0, c_buf=p32.c_buffer(), dtypes=p32.dtypes)
            GS.check_output(p32, c32, f"{what}, fp32 store")
            GS.check_bf16_store(clean[:M, :N].contiguous(), c32[:M, :N].contiguous(), what)


@pytest.mark.parametrize("N,K,tb", GS.LAYOUTS, ids=IDS)
def test_accumulate(kk, N, K, tb):
    """alpha = 1, beta = 1 onto a random fp32 C, plain and with the automatic k-slices (fp32 atomics)."""
    for math_mode, dtypes in GS.STORAGE:
        if dtypes & 4:
            continue
        for M in (1, 5, 17):
            p = GS.Problem(M, N, K, tb, math_mode, dtypes)
            run = Launcher(kk, p)
            A0, B0 = p.a_buffer(NAN).cuda(), p.b_buffer(NAN).cuda()
            for split in (1, 0):
                GS.check_values(run.accumulate(A0, B0, split), p.accumulate_reference(), *GS.accumulate_tolerance(K),
                                f"{p} accumulate, split_k = {split}")
