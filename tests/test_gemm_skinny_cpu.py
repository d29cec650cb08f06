"""The checker of the skinny-GEMM device tests (tests/gemm_skinny.py) against itself, without a GPU: it must accept a correct result
and reject subtly wrong ones, at the shapes, storage cases and tolerances test_gemm_skinny_gpu.py uses.

The stand-in for a device result is plain fp32 torch: an fp32 matmul of the operands rounded as the kernel sees them, plus bias and
the periodic residual, rounded to bf16 where C is stored so.  It is accepted at every (M, N, K, tb, storage) of the device tests, so
no tolerance is tighter than fp32 arithmetic allows.  Share of the bound that result uses, largest over all M and shapes (measured
against the fp64 reference; test_plain_fp32_result_is_accepted prints them):
  math 0 dtypes 0: 0.041     math 1 dtypes 0 / 2: 8.4e-5     math 1 dtypes 3: 1.9e-3     math 1 dtypes 7: 0.32
(dtypes 7 is the bf16 rounding of the result itself: half an ulp of |ref| against 0.1 + 1e-2 |ref|.)

Every mutation below is rejected at M = 5 and M = 17, for every shape and storage case, so no tolerance had to be tightened.  One
mutation cannot be shown at M = 5: with 5 rows and a period of 5, `row % (RES_MOD + 1)` names the same rows as `row % RES_MOD`;
there the neighbouring wrong period `row % (RES_MOD - 1)` is used (row 4 wraps to row 0), and at M = 17 both.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_skinny as GS  # noqa: E402

MUT_MS = (5, 17)
IDS = [f"N{N}-K{K}-tb{tb}" for N, K, tb in GS.LAYOUTS]


def _rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("N,K,tb", GS.LAYOUTS, ids=IDS)
def test_plain_fp32_result_is_accepted(N, K, tb):
    worst = {}
    for M in GS.MS:
        for math_mode, dtypes in GS.STORAGE:
            p = GS.Problem(M, N, K, tb, math_mode, dtypes)
            got = p.fp32_result()
            GS.check_output(p, p.c_buffer(got))
            ratio = GS.error_ratio(got, p.reference(), *GS.tolerance(math_mode, dtypes, K))
            worst[(math_mode, dtypes)] = max(worst.get((math_mode, dtypes), 0.0), ratio)
            if dtypes == 7:
                c32 = GS.Problem(M, N, K, tb, math_mode, 3).fp32_result()
                GS.check_bf16_store(got, c32, repr(p))
            if not p.c16 and M in (1, 5, 17):           # the accumulate form (alpha = 1, beta = 1, no bias, no residual)
                A, B = p.seen()
                GS.check_values(A @ B + p.acc, p.accumulate_reference(), *GS.accumulate_tolerance(K), f"{p} accumulate")
    print({k: f"{v:.2e}" for k, v in worst.items()})   # (the docstring's figures)


def _mutations(p):
    """(name, C buffer) of every wrong result whose value or sentinel check must fail."""
    M, N, K = p.M, p.N, p.K
    A, B = p.seen()
    out = []
    out.append(("last k element dropped", p.c_buffer(p.fp32_result(A=A[:, :K - 1], B=B[:K - 1]))))
    if K % 64:
        kf = K - K % 64
        out.append(("k tail beyond the last multiple of 64 dropped", p.c_buffer(p.fp32_result(A=A[:, :kf], B=B[:kf]))))
    periods = [GS.RES_MOD + 1] if M > GS.RES_MOD + 1 else []
    periods.append(GS.RES_MOD - 1)
    for period in periods:
        rows = p.rows(period)
        assert not torch.equal(rows, p.rows()), "the mutation must change something"
        out.append((f"residual row taken modulo {period}", p.c_buffer(p.fp32_result(rows=rows))))
    out.append(("bias shifted by one column", p.c_buffer(p.fp32_result(bias=torch.roll(p.bias, 1)))))
    for r in sorted({0, M - 2}):
        sw = p.fp32_result().clone()
        sw[[r, r + 1]] = sw[[r + 1, r]]
        out.append((f"rows {r} and {r + 1} swapped", p.c_buffer(sw)))
    good = p.fp32_result()
    row_past = p.c_buffer(good)
    row_past[M, :N] = good[M - 1]
    out.append(("one row of C beyond M written", row_past))
    col_past = p.c_buffer(good)
    col_past[:M, N] = good[:, N - 1]
    out.append(("one column beyond N written", col_past))
    one_past = p.c_buffer(good)
    one_past[M + GS.C_EXTRA_ROWS - 1, p.ldc - 1] = 7.5        # a single element, the last of the buffer
    out.append(("the last element of the buffer written", one_past))
    return out


@pytest.mark.parametrize("N,K,tb", GS.LAYOUTS, ids=IDS)
def test_subtly_wrong_results_are_rejected(N, K, tb):
    missed = []
    for M in MUT_MS:
        for math_mode, dtypes in GS.STORAGE:
            p = GS.Problem(M, N, K, tb, math_mode, dtypes)
            for name, cbuf in _mutations(p):
                if not _rejected(GS.check_output, p, cbuf):
                    missed.append((repr(p), name))
            if dtypes == 7:
                c32 = GS.Problem(M, N, K, tb, math_mode, 3).fp32_result()
                if not _rejected(GS.check_bf16_store, GS.truncate_bf16(c32), c32, repr(p)):
                    missed.append((repr(p), "bf16 output truncated instead of rounded"))
    assert not missed, missed


def test_period_mutation_is_void_at_five_rows():
    """Why M = 5 uses another wrong period: with as many rows as the period, row % (RES_MOD + 1) is row % RES_MOD."""
    p = GS.Problem(5, 80, 512, 0, 0, 0)
    assert torch.equal(p.rows(GS.RES_MOD + 1), p.rows())
    assert not torch.equal(p.rows(GS.RES_MOD - 1), p.rows())


def test_bit_checks_see_one_bit():
    a = torch.randn(7, 9)
    b = a.clone()
    GS.check_same_bits(a, b, "equal")
    b.view(torch.int32)[3, 4] ^= 1
    assert _rejected(GS.check_same_bits, a, b, "one bit")
    n = torch.full((2, 2), float("nan"))
    GS.check_same_bits(n, n.clone(), "NaN with the same bits is the same")
    assert _rejected(GS.check_values, n, torch.zeros(2, 2, dtype=torch.float64), 1.0, 1.0, "non-finite")
    c32 = torch.randn(64, 64) * 10
    GS.check_bf16_store(c32.bfloat16(), c32, "round to nearest even")
    assert _rejected(GS.check_bf16_store, GS.truncate_bf16(c32), c32, "truncation")


def test_embedding_geometry():
    """What the device test hands to kk_gemm: views from offset 0, 16-byte friendly leading dimensions, the fill only outside the view."""
    for N, K, tb in GS.LAYOUTS:
        for math_mode, dtypes in GS.STORAGE:
            p = GS.Problem(17, N, K, tb, math_mode, dtypes)
            assert p.lda == K + 16 and p.ldb == (N if tb else K) + 8 and p.ldc == N + 24 and p.ldr == N + 8
            assert p.lda % 8 == 0 and p.ldb % 8 == 0 and K % 8 == 0 and N % 8 == 0
            for fill in (0.0, float("nan")):
                a, b = p.a_buffer(fill), p.b_buffer(fill)
                assert tuple(a.shape) == (17 + 64, p.lda) and tuple(b.shape) == ((K if tb else N) + 64, p.ldb)
                assert torch.equal(a[:17, :K].float(), p.A) and torch.equal(b[:p.B.shape[0], :p.B.shape[1]].float(), p.B)
                for buf, (r, c) in ((a, p.A.shape), (b, p.B.shape)):
                    outside = torch.cat([buf[r:].flatten(), buf[:r, c:].flatten()]).float()
                    assert bool(torch.isnan(outside).all() if fill != fill else (outside == 0).all())
            r = p.r_buffer()
            assert torch.equal(r[:GS.RES_MOD, :N], p.res) and bool(torch.isnan(r[GS.RES_MOD:]).all())
            c = p.c_buffer()
            assert tuple(c.shape) == (17 + 8, p.ldc) and bool((c.float() == GS.SENTINEL).all())
