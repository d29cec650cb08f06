"""GPU suite: which kernel every public attention entry point launches, for small shapes on both sides of every gate of the host
dispatch (kk_attn.hip: storage, math, one tile / two groups, the 128-row block counts of the pair launch, the Sk cap, head-norm
descriptors, rope on the V descriptor, dropout and keep bits, the two-pass workspace).  The expected names (kk_last_kernel after the
call) are tests/golden/attn_routes.json, recorded by tools/record_attn_routes.py from the tree BEFORE a change to the dispatch: the
file is the memory of what the routes were, so a change that is meant to keep them never regenerates it.  Routes only: the numbers are test_kernels_gpu.py's, test_attn_v2_fp64_gpu.py's and test_keepgen_gpu.py's business.

Not covered here: operands off a 16-byte boundary (the fall-back kernels read 16-byte vectors through the same pointers, so no such
call is made; that column of the eligibility table in kk_attn.hip is covered by review)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_routes.json")

BF16, F32_BF16MATH, F32 = "bf16", "f32io_bf16math", "f32"      # storage / math
NO_HN, HN, HN_VROPE = "plain", "hn", "hn_vrope"                # head-norm descriptors: none, the engine's (rope on q and k), rope on v too


def _cases():
    """(B, h, Sq, Sk, causal, mode, hn, p_drop, forward_only)"""
    cs = []
    for S in (16, 33, 64, 65, 128, 129, 200):                                  # one tile | small | two groups; one | two 128-row blocks
        for causal in (0, 1):
            cs.append((1, 2, S, S, causal, BF16, NO_HN, 0.0, False))
    for Sq, Sk in ((40, 200), (200, 40), (130, 400)):                          # (the last: unequal block counts, no pair launch)
        cs.append((1, 2, Sq, Sk, 0, BF16, NO_HN, 0.0, False))
    cs.append((1, 2, 200, 130, 1, BF16, NO_HN, 0.0, False))                    # causal with Sq != Sk: no two-pass form
    cs.append((1, 2, 130, 4100, 0, BF16, NO_HN, 0.0, False))                   # Sk above 4096: dQ falls back, dK/dV does not
    for S, causal in ((64, 0), (200, 0), (200, 1)):                            # dropout (keep bits where the forward stores them)
        cs.append((1, 2, S, S, causal, BF16, NO_HN, 0.1, False))
    cs.append((1, 2, 130, 400, 0, BF16, NO_HN, 0.1, False))
    for S, causal in ((33, 0), (64, 1), (65, 1), (200, 0), (200, 1)):          # head-norm epilogues
        cs.append((1, 2, S, S, causal, BF16, HN, 0.0, False))
    cs.append((1, 2, 40, 200, 0, BF16, HN, 0.0, False))
    cs.append((1, 2, 200, 200, 1, BF16, HN, 0.1, False))
    for S, causal in ((64, 0), (200, 1)):                                      # rope on the V descriptor: the DMA-staged dK/dV refuses
        cs.append((1, 2, S, S, causal, BF16, HN_VROPE, 0.0, False))
    for S, causal in ((64, 0), (200, 0), (200, 1)):                            # fp32 storage, bf16 math
        cs.append((1, 2, S, S, causal, F32_BF16MATH, NO_HN, 0.0, False))
    cs.append((1, 2, 130, 400, 0, F32_BF16MATH, NO_HN, 0.1, False))
    cs.append((1, 2, 200, 200, 1, F32_BF16MATH, HN, 0.0, False))
    for S, causal, p in ((33, 0, 0.0), (200, 1, 0.0), (200, 0, 0.1)):          # fp32 math
        cs.append((1, 2, S, S, causal, F32, NO_HN, p, False))
    cs.append((1, 2, 40, 200, 0, F32, NO_HN, 0.0, False))
    cs.append((8, 8, 1024, 129, 0, BF16, NO_HN, 0.1, True))                    # two workgroups per CU with 128-query blocks: the q128 forward
    return cs


CASES = _cases()


def case_id(c):
    B, h, Sq, Sk, causal, mode, hn, p, fwd_only = c
    return f"{B}x{h}x{Sq}x{Sk}-{'causal' if causal else 'full'}-{mode}-{hn}-p{p}" + ("-fwd" if fwd_only else "")


def run_case(kk, c):
    """Walk one case through the entry points; {step: kernel name}."""
    B, h, Sq, Sk, causal, mode, hn, p, fwd_only = c
    lib = kk.load()
    H = h * 64
    io = 1 if mode == BF16 else 0
    math_ = kk.KK_MATH_F32 if mode == F32 else kk.KK_MATH_BF16
    dt = torch.bfloat16 if io else torch.float32
    torch.manual_seed(Sq * 7 + Sk)
    rnd = lambda rows, cols: (torch.randn(rows, cols, device="cuda") * 0.7).to(dt)
    q, kv, do = rnd(B * Sq, H), rnd(B * Sk, 2 * H), rnd(B * Sq, H)
    k, v = kv, kv[:, H:]
    o, lse = torch.zeros(B * Sq, H, device="cuda", dtype=dt), torch.zeros(B, h, Sq, device="cuda")
    seed = torch.tensor([77], dtype=torch.int32, device="cuda")
    site, scale = 5, 0.125
    routes = {}

    def step(name, entry, *args):
        kk.call(entry, *args)
        routes[name] = kk.last_kernel()

    fwd_args = (q, k, v, o, lse, B, h, Sq, Sk, H, 2 * H, 2 * H, H, None, causal, scale, seed, site, p, math_, io)
    nkeep = lib.kk_attn_keep_bytes(B, h, Sq, Sk) if (io and p > 0) else 0
    keep = torch.zeros(nkeep, dtype=torch.uint8, device="cuda") if nkeep > 0 else None
    step("fwd", "kk_attn_fwd", *fwd_args)
    step("fwd_kb", "kk_attn_fwd_kb", *fwd_args, keep)
    if keep is not None:
        step("fwd_rb", "kk_attn_fwd_rb", *fwd_args, keep)
    if fwd_only:
        torch.cuda.synchronize()
        return routes

    delta = torch.zeros(B, h, Sq, device="cuda")
    kk.call("kk_attn_delta", o, do, delta, B, h, Sq, H, H, io)
    dq, dkv = torch.zeros_like(q), torch.zeros_like(kv)
    hq = hkv = None
    if hn != NO_HN:
        raw_q, raw_kv = rnd(B * Sq, H), rnd(B * Sk, 2 * H)
        gains = [torch.ones(64, device="cuda") for _ in range(3)]
        pos = torch.arange(max(Sq, Sk), device="cuda", dtype=torch.float32)[:, None] * torch.linspace(1.0, 0.01, 64, device="cuda")[None, :]
        cos, sin = pos.cos().contiguous(), pos.sin().contiguous()
        pq = torch.zeros(1, lib.kk_attn_bwd_blocks(B, h, Sq), 64, device="cuda")
        pkv = torch.zeros(2, lib.kk_attn_bwd_blocks(B, h, Sk), 64, device="cuda")
        vrope = (cos, sin) if hn == HN_VROPE else (None, None)
        hq = kk.attn_headnorm([(raw_q, gains[0], pq[0], cos, sin)])
        hkv = kk.attn_headnorm([(raw_kv, gains[1], pkv[0], cos, sin), (raw_kv[:, H:], gains[2], pkv[1], *vrope)])

    tail = (None, causal, scale, seed, site, p, math_, io)
    step("bwd_dq", "kk_attn_bwd_dq", q, k, v, do, lse, delta, dq, B, h, Sq, Sk, H, 2 * H, 2 * H, H, H, *tail, None, 0, hq)
    step("bwd_dq_O", "kk_attn_bwd_dq", q, k, v, do, lse, delta, dq, B, h, Sq, Sk, H, 2 * H, 2 * H, H, H, *tail, o, H, hq)
    step("bwd_dkv", "kk_attn_bwd_dkv", q, k, v, do, lse, delta, dkv, dkv[:, H:], B, h, Sq, Sk, H, 2 * H, 2 * H, H, 2 * H, 2 * H, *tail, hkv)
    bwd_args = (q, k, v, do, lse, delta, dq, dkv, dkv[:, H:], B, h, Sq, Sk, H, 2 * H, 2 * H, H, H, 2 * H, 2 * H, *tail, hq, hkv)
    step("bwd", "kk_attn_bwd", *bwd_args)
    step("bwd_kb", "kk_attn_bwd_kb", *bwd_args, keep)
    need = lib.kk_attn_bwd_ws_bytes(B, h, Sq, Sk)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    step("bwd_ws", "kk_attn_bwd_ws", *bwd_args, ws, need)
    step("bwd_ws_small", "kk_attn_bwd_ws", *bwd_args, ws, need - 2048)
    torch.cuda.synchronize()
    return routes


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_recorded_cases_are_the_case_list(golden):
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) and sorted(golden) == sorted(ids)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_attention_routes_are_the_recorded_ones(kk, golden, case):
    assert run_case(kk, case) == golden[case_id(case)]
