"""GPU suite: which kernel every bf16 GEMM entry point launches (kk_last_kernel after the call), and the bits it leaves, for the
smallest shapes on both sides of every gate of the host dispatch in kk_gemm16.hip: the 128x128 and 128x64 tile counts, two or three
k-tiles, the large-tile family's K / N / alignment gates with row counts where its cost comparison goes each way, the split-K rules of
the plain route in all four operand layouts, and the grouped weight gradients' k-slices, overwrite, sweep direction and tile records.
The expected values are tests/golden/gemm_routes.json, recorded by tools/record_gemm_routes.py from the tree BEFORE a change to the
dispatch: the file is the memory of what the routes were, so a change that is meant to keep them never regenerates it.

Every case whose launch has no k-slices is deterministic, and the SHA-256 of its output tensors is compared as well: that catches a
change of stage count (another rounding order), of k_per_split and of a 1 -> n split.  Where a case IS k-sliced (fp32 atomics: the
order of the additions is not fixed) only the name is compared; the split count of those launches is covered by review of the
split-K block of kk_gemm16.hip, which moves as a block and is not rewritten.  Numbers against a reference are test_kernels_gpu.py's
and test_gemm_skinny_gpu.py's business."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.json")
BF = torch.bfloat16
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))                     # forward, dgrad, (A k-strided only), wgrad


def _plain(ta, tb, M, N, K, beta=0.0, c16=1, split_k=0, ldc_pad=0, sliced=False):
    return ("plain", ta, tb, M, N, K, beta, c16, split_k, ldc_pad, sliced)


def _cases():
    cs = []
    # ---- kk_gemm, bf16 x bf16 ----
    for ta, tb in LAYOUTS:                                      # 120 | 128 tiles of 128x64 (64x64 | eight waves), three k-tiles
        for N in (960, 1024):
            cs.append(_plain(ta, tb, 1024, N, 192, beta=0.0 if not ta else 1.0, c16=0 if ta else 1))
    for N in (960, 1024):                                       # ... and two k-tiles (two stages)
        cs.append(_plain(0, 0, 1024, N, 128))
    cs.append(_plain(1, 1, 1024, 1024, 200, beta=1.0, c16=0))  # the zero-filled K tail of the k-strided layout
    for N in (8064, 8192):                                      # 4032 | 4096 tiles of 128x128
        cs.append(_plain(0, 0, 8192, N, 64))
    for K in (960, 1024):                                       # the large-tile family: K gate x rows where the cost goes each way
        for M in (4090, 8192, 15996):
            for N in (512, 1000):
                cs.append(_plain(0, 0, M, N, K))
        for M, N in ((8192, 512), (4090, 1000)):
            cs.append(_plain(0, 1, M, N, K))
    cs.append(_plain(1, 1, 1024, 1024, 1024, beta=1.0, c16=0))  # (a weight-gradient layout never takes it)
    for ta, tb in LAYOUTS:                                      # split-K: 64 tiles (tiles * 2 <= 128) | 72 tiles
        cs.append(_plain(ta, tb, 512, 512, 1984, c16=0))                            # beta = 0, 31 k-tiles: not sliced
        cs.append(_plain(ta, tb, 512, 512, 2048, c16=0, sliced=True))               # beta = 0, 32 k-tiles
        cs.append(_plain(ta, tb, 512, 576, 2048, c16=0))                            # 72 tiles
        cs.append(_plain(ta, tb, 512, 512, 256, beta=1.0, c16=0, sliced=True))      # beta = 1: short reductions are sliced too
        cs.append(_plain(ta, tb, 512, 512, 128, beta=1.0, c16=0))                   # (two k-tiles: one slice)
        cs.append(_plain(ta, tb, 512, 512, 512, beta=1.0, c16=0, split_k=1))
        cs.append(_plain(ta, tb, 512, 512, 512, beta=1.0, c16=0, split_k=3, sliced=True))
        cs.append(_plain(ta, tb, 512, 512, 2048, c16=1))                            # a bf16 C is never sliced
        cs.append(_plain(ta, tb, 512, 512, 2048, c16=0, ldc_pad=8))                 # ldc != N at beta = 0: never sliced
        cs.append(_plain(ta, tb, 512, 512, 2048, c16=0, split_k=3, ldc_pad=8))
    # ---- kk_gemm_dgrad_delta (M, N, K, S) ----
    for M, N, K, S in ((256, 128, 128, 128), (256, 128, 192, 64), (4096, 512, 1024, 512), (8192, 512, 960, 1024), (8192, 512, 1024, 1024),
                       (4000, 320, 1024, 500)):
        cs.append(("delta", M, N, K, S))
    # ---- kk_gemm_dgrad_glu (T, F, H, p) ----
    for T, F, H, p in ((200, 96, 128, 0.0), (200, 96, 192, 0.1), (1024, 960, 192, 0.1), (1024, 1024, 192, 0.1), (1024, 1024, 128, 0.0),
                       (4096, 1536, 128, 0.2), (4096, 1536, 192, 0.2), (4000, 1000, 256, 0.1)):
        cs.append(("glu_bwd", T, F, H, p))
    # ---- kk_gemm_linear_glu (T, F, K, p) ----
    for T, F, K, p in ((64, 64, 64, 0.0), (333, 192, 128, 0.1), (333, 192, 192, 0.1), (1024, 960, 192, 0.0), (1024, 1024, 192, 0.1),
                       (4096, 1536, 128, 0.2), (4096, 1536, 192, 0.2), (8000, 1000, 256, 0.1)):
        cs.append(("glu_fwd", T, F, K, p))
    # ---- kk_gemm_qkv_headnorm (T, parts, heads, K, S, rope, ldraw pad, raw offset in elements) ----
    for T, parts, heads, K in ((1024, 3, 5, 192), (1024, 2, 8, 192), (1024, 2, 8, 128), (4096, 3, 8, 128), (4096, 3, 8, 192),
                               (8192, 3, 5, 192), (8192, 2, 8, 192), (8192, 2, 8, 128), (333, 3, 2, 192)):
        cs.append(("headnorm", T, parts, heads, K, T // 4 if T % 4 == 0 else T, 3, 0, 0))
    cs.append(("headnorm", 4096, 3, 8, 192, 512, 3, 4, 0))      # ldraw off a multiple of 8: no 16-byte stores
    cs.append(("headnorm", 8192, 2, 8, 192, 1024, 1, 0, 4))     # raw 8 bytes off a 16-byte boundary
    # ---- kk_gemm_wgrad_group (T, ((M, N), ...), split_k, overwrite, ss) ----
    big = ((512, 2048), (4096, 512), (512, 512), (1536, 512))   # 512 tiles of 128x64: the large tiles are cheaper
    for T in (960, 1024):
        for overwrite in (0, 1):
            cs.append(("group", T, big, 0, overwrite, 0))
    cs.append(("group", 1024, big, 2, 0, 0))
    cs.append(("group", 1024, big, 1, 0, 0))
    for T in (960, 1024):
        cs.append(("group", T, big, 0, 1, 1))                   # tile records: *ss_count afterwards
    cs.append(("group", 1024, ((512, 1024),), 0, 0, 0))         # 64 tiles: 2 * total <= 128, k-sliced
    cs.append(("group", 1024, ((512, 1088),), 0, 0, 0))         # 68 tiles
    cs.append(("group", 1024, ((512, 1024),), 0, 1, 0))         # (overwrite: never sliced)
    cs.append(("group", 1024, ((512, 1088),), 2, 0, 0))
    cs.append(("group", 520, ((128, 64),) * 8, 0, 0, 0))
    cs.append(("group", 520, ((128, 64),) * 8, 0, 1, 1))
    cs.append(("group", 1000, ((512, 192), (72, 64), (192, 512), (64, 136)), 0, 1, 1))      # M < N: the m-fastest sweep; N % 8 only
    cs.append(("group", 130, ((512, 1536), (200, 1000)), 0, 0, 0))                          # 3 k-tiles, a K tail
    return cs


CASES = _cases()


def case_id(c):
    if c[0] == "plain":
        _, ta, tb, M, N, K, beta, c16, split_k, ldc_pad, _ = c
        return f"plain-{ta}{tb}-{M}x{N}x{K}-beta{beta:g}-{'bf16' if c16 else 'f32'}-split{split_k}-pad{ldc_pad}"
    if c[0] == "group":
        _, T, shapes, split_k, overwrite, ss = c
        return f"group-{T}-" + "+".join(f"{m}x{n}" for m, n in shapes) + f"-split{split_k}-ow{overwrite}-ss{ss}"
    return "-".join(str(v) for v in c)


def group_sliced(c):
    """k-slices of a grouped launch, restated from the entry point's contract: the caller's count, else enough to bring
    2 * (128x64 tiles) up to 128 workgroups; never with overwrite."""
    _, T, shapes, split_k, overwrite, _ = c
    total = sum(-(-m // 128) * -(-n // 64) for m, n in shapes)
    return not overwrite and (split_k > 1 or (split_k <= 0 and total * 2 <= 128)) and -(-T // 64) >= 4


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


_POOL = {}


def _rnd(g, *shape, scale=1.0):
    """Reproducible N(0, scale) values: a window sequence over one million CPU-generated numbers (the big operands here would take
    longer to draw on the host than every launch of this file together).  g: [next offset], advanced by the call."""
    if "p" not in _POOL:
        _POOL["p"] = torch.randn(1000003, generator=torch.Generator().manual_seed(1234)).to("cuda")
    n = 1
    for v in shape:
        n *= v
    idx = (torch.arange(n, device="cuda") + g[0]) % 1000003
    g[0] = (g[0] + n + 7919) % 1000003
    return (_POOL["p"][idx] * scale).view(*shape)


def run_case(kk, c):
    """One call of the entry point; {"kernel": name[, "sha256": digest of the outputs][, "ss_count": records left]}."""
    g = [sum(int(v) for v in c[1:] if isinstance(v, int)) % 1000003]
    seed = torch.tensor([21], dtype=torch.int32, device="cuda")
    out, outs, sliced = {}, (), False
    if c[0] == "plain":
        _, ta, tb, M, N, K, beta, c16, split_k, ldc_pad, sliced = c
        A = _rnd(g, *((K, M) if ta else (M, K))).to(BF)
        B = _rnd(g, *((K, N) if tb else (N, K)), scale=0.1).to(BF)
        Cm = _rnd(g, M, N + ldc_pad) if beta != 0.0 or ldc_pad else torch.full((M, N), 7.0, device="cuda")      # (what beta = 0 must not read)
        Cm = Cm.to(BF if c16 else torch.float32)
        kk.call("kk_gemm", ta, tb, M, N, K, 1.0, A, A.stride(0), B, B.stride(0), beta, Cm, N + ldc_pad, None, None, 0, 0, split_k, 1,
                3 + 4 * c16)
        outs = (Cm,)
    elif c[0] == "delta":
        _, M, N, K, S = c
        dy, W, o = _rnd(g, M, K).to(BF), _rnd(g, K, N, scale=0.1).to(BF), _rnd(g, M, N).to(BF)
        dx, delta = torch.full((M, N), 7.0, device="cuda", dtype=BF), torch.full((M // S, N // 64, S), 7.0, device="cuda")
        assert kk.load().kk_gemm_dgrad_delta_supported(M, N, K)
        kk.call("kk_gemm_dgrad_delta", M, N, K, dy, K, W, N, dx, N, o, N, delta, S, N // 64)
        outs = (dx, delta)
    elif c[0] == "glu_bwd":
        _, T, F, H, p = c
        dy, W, h1 = _rnd(g, T, H).to(BF), _rnd(g, H, F, scale=0.1).to(BF), _rnd(g, T, 2 * F).to(BF)
        part = torch.full((kk.load().kk_gemm_dgrad_glu_blocks(T), 2 * F), 4.0, device="cuda")
        dh = torch.full((T, 2 * F), 7.0, device="cuda", dtype=BF)
        kk.call("kk_gemm_dgrad_glu", T, F, H, dy, H, W, h1, dh, part, seed, 9, p)
        outs = (dh, part)
    elif c[0] == "glu_fwd":
        _, T, F, K, p = c
        x, W, b = _rnd(g, T, K).to(BF), _rnd(g, 2 * F, K, scale=0.1).to(BF), _rnd(g, 2 * F)
        h1, gate = torch.full((T, 2 * F), 7.0, device="cuda", dtype=BF), torch.full((T, F), 7.0, device="cuda", dtype=BF)
        kk.call("kk_gemm_linear_glu", T, F, K, x, K, W, b, h1, gate, F, seed, 13, p)
        outs = (h1, gate)
    elif c[0] == "headnorm":
        _, T, parts, heads, K, S, rope, pad, off = c
        N = parts * heads * 64
        x, W = _rnd(g, T, K).to(BF), _rnd(g, N, K, scale=0.1).to(BF)
        gains = [1.0 + 0.2 * _rnd(g, 64) for _ in range(parts)]
        cos, sin = _rnd(g, S, 64).clamp(-1, 1), _rnd(g, S, 64).clamp(-1, 1)      # (tables of the right shape: the bits are compared, not the rotation)
        raw_buf = torch.full((T * (N + pad) + 8,), 7.0, device="cuda", dtype=BF)
        raw = raw_buf[off:off + T * (N + pad)].view(T, N + pad)
        y = torch.full((T, N), 7.0, device="cuda", dtype=BF)
        kk.call("kk_gemm_qkv_headnorm", T, parts, heads, K, x, K, W, None, raw, N + pad, y, N, S, kk.pointer_table(gains), rope, cos, sin)
        outs = (raw_buf, y)
    else:
        _, T, shapes, split_k, overwrite, ss = c
        probs = []
        for M, N in shapes:
            wide = _rnd(g, T, M + 8).to(BF)                     # a strided view, like a slice of the fused q|k|v gradient
            probs.append((wide[:, 8:], _rnd(g, T, N).to(BF), _rnd(g, M, N)))
        n = len(probs)
        lib = kk.load()
        rec = torch.zeros(lib.kk_seg_sumsq_rec_capacity() * 16, dtype=torch.uint8, device="cuda") if ss else None
        seg = (ctypes.c_int32 * (2 * n))(*[v for i in range(n) for v in (i, 0)]) if ss else None
        count = (ctypes.c_int32 * 1)(3) if ss else None
        kk.call("kk_gemm_wgrad_group", kk.wgrad_table(probs), n, split_k, overwrite, rec, seg, count)
        outs = tuple(dw for _, _, dw in probs) + ((rec,) if ss else ())
        sliced = group_sliced(c)
        if ss:
            out["ss_count"] = int(count[0])
    out["kernel"] = kk.last_kernel()
    torch.cuda.synchronize()
    if not sliced:
        out["sha256"] = _digest(*outs)
    return out


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
    assert sum("sha256" not in v for v in golden.values()) == sum(1 for c in CASES if (c[0] == "plain" and c[-1]) or (c[0] == "group" and group_sliced(c)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gemm_routes_and_bits_are_the_recorded_ones(kk, golden, case):
    assert run_case(kk, case) == golden[case_id(case)]
