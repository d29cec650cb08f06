"""GPU suite, kernel level: the decode step's state kernels of kk_decode.hip in both forms, lockstep (KokoroEngine.generate,
generate_batch) and per slot (generate_stream), and the row form of the decode attention (kk_attn_decode_rows, kk_attn_fwd.hip).  The row
attention against a float64 softmax and, bit for bit, against kk_attn_fwd at Sq = 1 over the same live keys: a key count and the
equivalent key mask select the same arithmetic in one kernel.  Prologue, cache append, epilogue and slot admission against plain torch
indexing.  (The lockstep epilogue with the stop rule: test_synth_kernels_gpu.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, HEADS, CAP = 4, 8, 520
KLEN = [0, 1, 257, 520]          # an empty row, one key, one key past a group wrap (256), a full cache that is no multiple of 256
H = HEADS * 64


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def _qkv(bf16, seed=0, nan_tail=True):
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if bf16 else torch.float32
    q = torch.randn(S, H, generator=g).cuda().to(dt)
    K, V = torch.randn(S, CAP, H, generator=g).cuda().to(dt), torch.randn(S, CAP, H, generator=g).cuda().to(dt)
    live = torch.arange(CAP)[None, :] < torch.tensor(KLEN)[:, None]                 # [S, CAP]
    if nan_tail:
        K[~live.cuda()] = float("nan")
        V[~live.cuda()] = float("nan")
    return q, K, V, live


def _rows(kk, q, K, V, klen, mask, bf16, k_slot=None, ldk=None):
    out = torch.full((S, H), 7.0, device="cuda", dtype=q.dtype)
    lse = torch.full((S, HEADS), 7.0, device="cuda")
    k_slot, ldk = (CAP * H, H) if k_slot is None else (k_slot, ldk)
    kk.call("kk_attn_decode_rows", q, K, V, out, lse, klen, mask, S, HEADS, CAP, k_slot, ldk, k_slot, ldk, 0.125, 1 if bf16 else 0)
    torch.cuda.synchronize()
    return out, lse


def _fp64(q, K, V, masked):
    """softmax(q.K^T / 8).V in float64 over the keys that are not `masked` [S, CAP] (masked keys may hold NaN); lse."""
    qd = q.double().cpu().view(S, HEADS, 64)
    Kd = K.double().cpu().view(S, CAP, HEADS, 64).masked_fill(masked[:, :, None, None], 0.0)
    Vd = V.double().cpu().view(S, CAP, HEADS, 64).masked_fill(masked[:, :, None, None], 0.0)
    s = torch.einsum("bhd,bkhd->bhk", qd, Kd) * 0.125
    s = s.masked_fill(masked[:, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)
    return torch.einsum("bhk,bkhd->bhd", p, Vd).reshape(S, H), torch.logsumexp(s, dim=-1)


def _check_fp64(out, lse, ref, ref_lse, masked, bf16):
    # the bounds of test_attention_decode_step for attn_decode_kernel
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=2e-2 if bf16 else 2e-5, rtol=1e-2 if bf16 else 1e-5)
    alive = ~masked.all(dim=1)
    torch.testing.assert_close(lse.cpu()[alive], ref_lse[alive].float(), atol=1e-4, rtol=1e-5)
    for s in range(S):
        if not alive[s]:
            assert bool((out[s] == 0).all()) and bool(torch.isinf(lse[s]).all()) and bool((lse[s] > 0).all())


def _attn_fwd(kk, q, K, V, masked, bf16):
    """kk_attn_fwd at Sq = 1 (attn_decode_kernel) over a zeroed tail under the equivalent key mask."""
    K0, V0 = K.clone(), V.clone()
    K0[masked.cuda()] = 0
    V0[masked.cuda()] = 0
    out, lse = torch.empty(S, H, device="cuda", dtype=q.dtype), torch.empty(S, HEADS, 1, device="cuda")
    kk.call("kk_attn_fwd", q, K0, V0, out, lse, S, HEADS, 1, CAP, H, H, H, H, masked.to(torch.uint8).cuda(), 0, 0.125, None, 0, 0.0,
            1 if bf16 else 0, 1 if bf16 else 0)
    torch.cuda.synchronize()
    return out, lse.view(S, HEADS)


@pytest.mark.parametrize("bf16", [False, True])
def test_attn_decode_rows_against_fp64_and_attn_fwd(kk, bf16):
    """Keys at or past klen[s] are NaN: nothing of them may be loaded.  Row by row the bits of kk_attn_fwd at Sq = 1."""
    q, K, V, live = _qkv(bf16)
    klen = torch.tensor(KLEN, dtype=torch.int32).cuda()
    out, lse = _rows(kk, q, K, V, klen, None, bf16)
    assert bool(torch.isfinite(out.float()).all())
    ref, ref_lse = _fp64(q, K, V, ~live)
    _check_fp64(out, lse, ref, ref_lse, ~live, bf16)
    out2, lse2 = _attn_fwd(kk, q, K, V, ~live, bf16)
    for s in range(S):
        assert torch.equal(out[s], out2[s]), f"row {s}: output bits"
        assert torch.equal(lse[s], lse2[s]), f"row {s}: lse bits"


@pytest.mark.parametrize("bf16", [False, True])
def test_attn_decode_rows_with_key_mask_in_the_pool_layout(kk, bf16):
    """The cross-attention form: K | V are column slices of one [S*cap, 2H*layers] pool, a key mask [S, cap] on top of the key count."""
    q, K, V, live = _qkv(bf16, seed=1)
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(S, CAP, generator=g) < 0.3
    mask[:, 0] = False
    mask[2, :257] = True                                       # every live key of row 2 masked: zero output, lse = +inf
    layers, W = 2, 4 * H
    pool = torch.full((S * CAP, W), float("nan"), device="cuda", dtype=q.dtype)
    pool[:, 2 * H:3 * H], pool[:, 3 * H:] = K.view(S * CAP, H), V.view(S * CAP, H)
    klen = torch.tensor(KLEN, dtype=torch.int32).cuda()
    out, lse = _rows(kk, q, pool[:, 2 * H:], pool[:, 3 * H:], klen, mask.to(torch.uint8).cuda(), bf16, k_slot=CAP * W, ldk=W)
    masked = mask | ~live
    ref, ref_lse = _fp64(q, K, V, masked)
    _check_fp64(out, lse, ref, ref_lse, masked, bf16)
    out2, lse2 = _attn_fwd(kk, q, K, V, masked, bf16)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


# ---------------------------------------------------------------------------------------------------------------- state kernels
N_POS, M, HS = 64, 20, 128           # positional rows, mel channels, hidden of the state tests
CAP2, L1 = 40, 41
T_ROWS = [0, 7, 33, 39, 12, 31, 35]
DONE = [0, 0, 0, 0, 1, 0, 0]
S2 = len(T_ROWS)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32).cuda()


@pytest.mark.parametrize("t", [0, 5, 7])                       # 7 = L1 - 2, the last legal frame
def test_decode_prologue(kk, t):
    """The lockstep form, one workgroup: B * M = 280 and H = 320 reach the second pass of its 256-thread loops."""
    n_pos, l1, m, h, b = 16, 9, 20, 320, 14
    g = torch.Generator().manual_seed(2)
    mel_all = torch.randn(b, l1, m, generator=g).cuda()
    pe, cos, sin = (torch.randn(n_pos, n, generator=g).cuda() for n in (h, 64, 64))
    frame_in, pe_row, cos_row, sin_row = (torch.full(sh, 9.0, device="cuda") for sh in ((b, m), (h,), (64,), (64,)))
    mask0 = torch.arange(1, l1, dtype=torch.uint8)              # every key still hidden, each byte its own value
    key_mask, t_dev = mask0.clone().cuda(), _i32([t])
    kk.call("kk_decode_prologue", mel_all, frame_in, pe, pe_row, cos, sin, cos_row, sin_row, key_mask, t_dev, b, l1, m, h)
    torch.cuda.synchronize()
    assert torch.equal(frame_in, mel_all[:, t]) and torch.equal(pe_row, pe[t])
    assert torch.equal(cos_row, cos[t]) and torch.equal(sin_row, sin[t])
    want_mask = mask0.clone()
    want_mask[t] = 0
    assert torch.equal(key_mask.cpu(), want_mask)
    assert t_dev.item() == t


def test_decode_prologue_rows(kk):
    g = torch.Generator().manual_seed(3)
    mel_all = torch.randn(S2, L1, M, generator=g).cuda()
    pe, cos, sin = (torch.randn(N_POS, n, generator=g).cuda() for n in (HS, 64, 64))
    frame_in, pe_rows, cos_rows, sin_rows = (torch.full((S2, n), 9.0, device="cuda") for n in (M, HS, 64, 64))
    klen = torch.full((S2,), -5, dtype=torch.int32, device="cuda")
    t, done = _i32(T_ROWS), _i32(DONE)
    kk.call("kk_decode_prologue_rows", mel_all, frame_in, pe, pe_rows, cos, sin, cos_rows, sin_rows, t, done, klen, S2, L1, M, HS, N_POS)
    torch.cuda.synchronize()
    pos = [0 if d else ts for ts, d in zip(T_ROWS, DONE)]      # a finished row is fed position 0
    for s, p in enumerate(pos):
        assert torch.equal(frame_in[s], mel_all[s, p]) and torch.equal(pe_rows[s], pe[p])
        assert torch.equal(cos_rows[s], cos[p]) and torch.equal(sin_rows[s], sin[p])
    assert klen.tolist() == [0 if d else ts + 1 for ts, d in zip(T_ROWS, DONE)]
    assert t.tolist() == T_ROWS and done.tolist() == DONE


@pytest.mark.parametrize("t", [0, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_decode_cache_append(kk, bf16, t):
    """The lockstep form over time-major caches [L][B * H]: B * H = 384 takes two workgroups."""
    b, h, rows = 3, 128, 6
    dt = torch.bfloat16 if bf16 else torch.float32
    nrm = torch.randn(b, 3 * h, generator=torch.Generator().manual_seed(9)).cuda().to(dt)
    q, Kc, Vc = (torch.full(sh, 7.0, device="cuda", dtype=dt) for sh in ((b * h,), (rows, b * h), (rows, b * h)))
    kk.call("kk_decode_cache_append", nrm, q, Kc, Vc, _i32([t]), b, h, 1 if bf16 else 0)
    torch.cuda.synchronize()
    assert torch.equal(q, nrm[:, :h].reshape(-1))
    for cache, lo in ((Kc, h), (Vc, 2 * h)):
        want = torch.full_like(cache, 7.0)                     # every other row still holds the sentinel
        want[t] = nrm[:, lo:lo + h].reshape(-1)
        assert torch.equal(cache, want)


@pytest.mark.parametrize("bf16", [False, True])
def test_decode_cache_append_rows(kk, bf16):
    g = torch.Generator().manual_seed(4)
    dt = torch.bfloat16 if bf16 else torch.float32
    nrm = torch.randn(S2, 3 * HS, generator=g).cuda().to(dt)
    q0, Kc0, Vc0 = (torch.randn(*sh, generator=g).cuda().to(dt) for sh in ((S2, HS), (S2, CAP2, HS), (S2, CAP2, HS)))
    q, Kc, Vc = q0.clone(), Kc0.clone(), Vc0.clone()
    kk.call("kk_decode_cache_append_rows", nrm, q, Kc, Vc, _i32(T_ROWS), _i32(DONE), S2, CAP2, HS, 1 if bf16 else 0)
    torch.cuda.synchronize()
    wq, wk, wv = q0.clone(), Kc0.clone(), Vc0.clone()
    for s, (ts, d) in enumerate(zip(T_ROWS, DONE)):
        if not d:
            wq[s], wk[s, ts], wv[s, ts] = nrm[s, :HS], nrm[s, HS:2 * HS], nrm[s, 2 * HS:]
    assert torch.equal(q, wq) and torch.equal(Kc, wk) and torch.equal(Vc, wv)       # (the finished row 4: byte-identical)


def test_decode_epilogue(kk):
    """The lockstep form without a stop rule, one workgroup: B = 260 reaches the second pass of the stop-logit loop (and B * M = 520
    the third of the frame loop)."""
    b, m, l1, t = 260, 2, 5, 2
    g = torch.Generator().manual_seed(7)
    frame_out, stop = torch.randn(b, m, generator=g).cuda(), torch.randn(b, generator=g).cuda()
    mel_all, stop_all = torch.full((b, l1, m), 7.0, device="cuda"), torch.full((l1 - 1, b), 7.0, device="cuda")
    t_dev = _i32([t])
    kk.call("kk_decode_epilogue", frame_out, stop, mel_all, stop_all, t_dev, b, l1, m)
    torch.cuda.synchronize()
    want_mel, want_stop = torch.full_like(mel_all, 7.0), torch.full_like(stop_all, 7.0)
    want_mel[:, t + 1], want_stop[t] = frame_out, stop
    assert torch.equal(mel_all, want_mel) and torch.equal(stop_all, want_stop)
    assert t_dev.item() == t + 1


def test_decode_epilogue_slots(kk):
    """Row 0 stops by the threshold, row 2 by the quiet output, row 3 by max_b, row 5 by the post-expected threshold; rows 1 and 6
    go on (1 with the stop head firing below its min, 6 past frame 30 with a loud output); row 4 is finished and must stay
    byte-identical."""
    g = torch.Generator().manual_seed(6)
    mel0 = torch.randn(S2, L1, M, generator=g)
    mel0[2, 5:34] = -10.0                                      # rows t - 28 .. t of slot 2 (t = 33)
    frame_out = torch.randn(S2, M, generator=g)
    frame_out[2] = -10.0
    stop = torch.tensor([5.0, 5.0, -5.0, -5.0, 5.0, 0.0, -5.0])
    min_b = [0, 8, 0, 100, 0, 0, 0]
    exp_b = [10, 10, 40, 40, 10, 20, 40]
    max_b = [40, 40, 40, 40, 40, 40, 40]
    stop_all0 = torch.randn(S2, CAP2, generator=g)
    mel, stop_all = mel0.clone().cuda(), stop_all0.clone().cuda()
    t, done, frames = _i32(T_ROWS), _i32(DONE), _i32([0, 0, 0, 0, 13, 0, 0])
    live = _i32([6])
    kk.call("kk_decode_epilogue_slots", frame_out.cuda(), stop.cuda(), mel, stop_all, t, done, frames, live, _i32(min_b), _i32(exp_b),
            _i32(max_b), S2, L1, M, 0.9, 0.2)
    torch.cuda.synchronize()
    want_mel, want_stop = mel0.clone(), stop_all0.clone()
    for s, (ts, d) in enumerate(zip(T_ROWS, DONE)):
        if not d:
            want_mel[s, ts + 1] = frame_out[s]
            want_stop[s, ts] = stop[s]
    assert torch.equal(mel.cpu(), want_mel) and torch.equal(stop_all.cpu(), want_stop)
    assert t.tolist() == [1, 8, 34, 40, 12, 32, 36]            # += 1 for live rows only
    assert done.tolist() == [1, 0, 1, 1, 1, 1, 0]
    assert frames.tolist() == [1, 0, 34, 40, 13, 32, 0]
    assert live.item() == 2


@pytest.mark.parametrize("bf16", [False, True])
def test_slot_admit(kk, bf16):
    g = torch.Generator().manual_seed(8)
    dt = torch.bfloat16 if bf16 else torch.float32
    n, T_adm, W = 2, 9, 2 * HS * 3
    slots = [4, 1]
    kv_src = torch.randn(n * T_adm, W, generator=g).cuda().to(dt)
    pool0 = torch.randn(S2 * CAP2, W, generator=g).cuda().to(dt)
    fm_src = (torch.rand(n, T_adm, generator=g) < 0.4).to(torch.uint8).cuda()
    fm0 = (torch.rand(S2, CAP2, generator=g) < 0.5).to(torch.uint8).cuda()
    mel0 = torch.randn(S2, L1, M, generator=g).cuda()
    state0 = torch.randint(1, 30, (8, S2), generator=g).to(torch.int32).cuda()      # t | done | frames | clen | min | expected | max | (spare)
    bounds = torch.tensor([[3, 4], [9, 8], [30, 25]], dtype=torch.int32).cuda()
    pool, fm, mel, st, live = pool0.clone(), fm0.clone(), mel0.clone(), state0.clone(), _i32([3])
    kk.call("kk_slot_admit", kv_src, pool, fm_src, fm, _i32(slots), bounds, st[0], st[1], st[2], st[3], st[4], st[5], st[6], mel, live,
            n, T_adm, S2, CAP2, W * kv_src.element_size(), L1, M)
    torch.cuda.synchronize()
    wp, wf, wm, ws = pool0.clone(), fm0.clone(), mel0.clone(), state0.clone()
    for r, s in enumerate(slots):
        wp[s * CAP2:s * CAP2 + T_adm] = kv_src[r * T_adm:(r + 1) * T_adm]
        wf[s, :T_adm], wf[s, T_adm:] = fm_src[r], 1
        wm[s, 0] = 0
        ws[:7, s] = torch.tensor([0, 0, 0, T_adm, int(bounds[0, r]), int(bounds[1, r]), int(bounds[2, r])], dtype=torch.int32).cuda()
    assert torch.equal(pool, wp) and torch.equal(fm, wf) and torch.equal(mel, wm) and torch.equal(st, ws)
    assert live.item() == 5
