"""GPU suite, kernel level: the batched-synthesis kernels (KokoroEngine.generate_batch: the variance predictors' kernels with the rows'
lengths, the decode epilogue of kk_decode.hip) against plain torch restatements of what each row would get at B = 1."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CHUNK = 512


@pytest.fixture(scope="module")
def kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib
    lib.load()
    return lib


def _ref_im2col3_rows(x, lens, L, C):
    """[B*L, 3C] operand of conv1d(k=3, padding=1) per 512-frame chunk, where a tap at a position >= lens[b] (or outside the
    chunk) reads zero: on rows l < lens[b], the operand of the B = 1 convolution over the row's first lens[b] frames."""
    B = len(lens)
    xv = x.view(B, L, C)
    col = torch.zeros(B, L, C, 3)
    l = torch.arange(L)
    cb = (l // CHUNK) * CHUNK
    for b, n in enumerate(lens):
        ce = torch.clamp(cb + CHUNK, max=min(L, n))
        for k in range(3):
            pos = l + k - 1
            ok = (pos >= cb) & (pos < ce)
            col[b, ok, :, k] = xv[b, pos[ok]]
    return col.view(B * L, 3 * C)


def _lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("bf16", [False, True])
def test_im2col3_rows_fwd(kk, bf16):
    lens, L, C = [1, 2, 511, 512, 513, 1100], 1100, 24
    B = len(lens)
    x = torch.randn(B * L, C, generator=torch.Generator().manual_seed(1))
    col = torch.full((B * L, 3 * C), 7.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    kk.call("kk_im2col3_fwd", x.cuda(), col, _lens_t(lens), B, L, C, CHUNK, 1 if bf16 else 0)
    ref = _ref_im2col3_rows(x, lens, L, C)
    if bf16:
        ref = ref.to(torch.bfloat16)
    assert torch.equal(col.cpu(), ref), "bit-exact"


def test_im2col3_rows_equals_the_plain_kernel_at_full_length(kk):
    """Rows of full length: exactly kk_im2col3_fwd without lens."""
    B, L, C = 3, 700, 16
    x = torch.randn(B * L, C, generator=torch.Generator().manual_seed(2)).cuda()
    a, b = torch.empty(B * L, 3 * C, device="cuda"), torch.empty(B * L, 3 * C, device="cuda")
    kk.call("kk_im2col3_fwd", x, a, None, B, L, C, CHUNK, 0)
    kk.call("kk_im2col3_fwd", x, b, _lens_t([L] * B), B, L, C, CHUNK, 0)
    assert torch.equal(a, b)


def test_groupnorm_relu_rows_fwd(kk):
    # 513: the last chunk holds exactly one valid frame (zeros); 1: a one-frame row (zeros); 1025: 512 + 512 + 1
    lens, L, C = [1, 2, 511, 512, 513, 1025, 1100, 700], 1100, 32
    B = len(lens)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * L, C, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.2
    nch = -(-L // CHUNK)
    y = torch.full((B * L, C), 9.0, device="cuda")
    stats = torch.empty(B * nch, 2, device="cuda")
    scratch = torch.full((2 * B * nch,), float("nan"), dtype=torch.float64, device="cuda")      # the call zeroes it itself
    kk.call("kk_groupnorm_relu_fwd", x.cuda(), gamma.cuda(), beta.cuda(), y, stats, scratch, _lens_t(lens), B, L, C, CHUNK,
            None, 0, 0.0)
    assert float(scratch.abs().max()) == 0.0, "the scratch is handed back zeroed"
    ref = torch.zeros(B, L, C)
    xv = x.view(B, L, C)
    for b, n in enumerate(lens):
        for s in range(0, n, CHUNK):
            seg = xv[b, s:min(s + CHUNK, n)]
            if seg.shape[0] < 2:
                continue
            h = F.group_norm(seg.t()[None], 1, gamma, beta, 1e-5)
            ref[b, s:s + seg.shape[0]] = F.relu(h)[0].t()
    got = y.cpu().view(B, L, C)
    torch.testing.assert_close(got, ref, atol=2e-4, rtol=2e-4)
    assert float(got[4, 512].abs().max()) == 0.0 and float(got[0].abs().max()) == 0.0, "degenerate chunks are zeros"
    assert float(got[2, 511:].abs().max()) == 0.0, "positions past the row's length are zeros"


def test_groupnorm_relu_rows_equals_the_plain_kernel_at_full_length(kk):
    """lens = [L] * B against lens = None, bit for bit in y and stats.  The input is multiples of 0.25 in [-2, 2]: every fp32 partial
    sum (<= 2048 terms of at most 2, resp. 4 = 64 quarter-squares, far below 2^24 units of 1/16) and every fp64 sum is exact, so the
    order in which the fp64 atomics arrive cannot change a bit and equality is a fair demand."""
    B, L, C, chunk = 3, 513, 32, 512
    g = torch.Generator().manual_seed(6)
    x = (torch.randint(-8, 9, (B * L, C), generator=g).float() * 0.25).cuda()
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1.0).cuda(), (torch.randn(C, generator=g) * 0.2).cuda()
    nch = -(-L // chunk)
    res = []
    for lens in (None, _lens_t([L] * B)):
        y, stats = torch.full((B * L, C), 9.0, device="cuda"), torch.full((B * nch, 2), 9.0, device="cuda")
        scratch = torch.full((2 * B * nch,), float("nan"), dtype=torch.float64, device="cuda")
        kk.call("kk_groupnorm_relu_fwd", x, gamma, beta, y, stats, scratch, lens, B, L, C, chunk, None, 0, 0.0)
        assert float(scratch.abs().max()) == 0.0
        res.append((y, stats))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][0].abs().max()) > 0.0


def _ref_row_mask(mask_in, lens, L):
    """The rows of a predictor's Linear(C->1) that are filled with 0: padding, frames past the row's length, chunks of < 2 valid frames."""
    ref = mask_in.bool().clone() if mask_in is not None else torch.zeros(len(lens), L, dtype=torch.bool)
    for b, n in enumerate(lens):
        ref[b, n:] = True
        for s in range(0, n, CHUNK):
            if min(s + CHUNK, n) - s < 2:
                ref[b, s:s + CHUNK] = True
    return ref


def test_varpred_row_mask(kk):
    """kk_rowdot_fwd with lens: with w = 0 and b = 1 the output IS the complement of the row mask, element for element."""
    lens, L, C = [1, 2, 511, 513, 600, 1025], 1100, 8
    B = len(lens)
    g = torch.Generator().manual_seed(4)
    mask_in = (torch.rand(B, L, generator=g) < 0.1).to(torch.uint8)
    x = torch.randn(B * L, C, generator=g).cuda()
    w0, b1 = torch.zeros(C, device="cuda"), torch.ones(1, device="cuda")
    for m in (mask_in, None):
        out = torch.full((B, L), 5.0, device="cuda")
        kk.call("kk_rowdot_fwd", x, w0, b1, m.cuda() if m is not None else None, _lens_t(lens), out, B * L, C, L, CHUNK, 0)
        ref = _ref_row_mask(m, lens, L)
        assert torch.equal(out.cpu(), (~ref).float()), "exactly 0.0 on the masked rows, exactly 1.0 elsewhere"
    # a random w: x @ w + b on the live rows, in float64 (atol = rtol = 1e-5: the rowdot's own tolerance in test_kernels_gpu.py)
    w, bias = torch.randn(C, generator=g), torch.randn(1, generator=g)
    out = torch.full((B, L), 5.0, device="cuda")
    kk.call("kk_rowdot_fwd", x, w.cuda(), bias.cuda(), mask_in.cuda(), _lens_t(lens), out, B * L, C, L, CHUNK, 0)
    dead = _ref_row_mask(mask_in, lens, L)
    ref = (x.cpu().double() @ w.double() + bias.double()).view(B, L).masked_fill(dead, 0.0)
    torch.testing.assert_close(out.cpu().double(), ref, atol=1e-5, rtol=1e-5)
    assert float(out.cpu()[dead].abs().max()) == 0.0


def _ref_stop_rule(frames, logits, bounds, thr, post, steps):
    """model/generator.py:67-88 applied to each row alone: (frames_b, or 0 when the row is still live after `steps` frames)."""
    B = logits.shape[1]
    out = [0] * B
    for b in range(B):
        lo, ex, hi = bounds[b]
        for t in range(steps):
            stop = t + 1 >= hi
            if not stop and t >= lo:
                th = thr if t < ex else min(thr, post)
                p = 1.0 / (1.0 + math.exp(-float(logits[t, b])))
                if p > th:
                    stop = True
                elif t + 1 >= 30 and float(frames[t - 29:t + 1, b].double().mean()) < -9.5:
                    stop = True
            if stop:
                out[b] = t + 1
                break
    return out


def test_decode_epilogue_rows(kk):
    steps, B, M = 80, 6, 8
    thr, post = 0.5, 0.2
    frames = torch.randn(steps, B, M, generator=torch.Generator().manual_seed(5)) * 0.1
    p = torch.full((steps, B), 0.05)
    bounds = [None] * B
    # 0: fires at t = 10, before expected
    bounds[0] = (5, 20, 60)
    p[10:, 0] = 0.9
    # 1: p = 0.35 from t = 15: below the threshold before expected, above the lowered one from t = expected = 20
    bounds[1] = (5, 20, 60)
    p[15:, 1] = 0.35
    # 2: passes the threshold before min (ignored), fires at t = 45
    bounds[2] = (30, 40, 70)
    p[:30, 2] = 0.9
    p[45:, 2] = 0.9
    # 3: the 30-frame energy rule: -4 for t < 15, -10 after; the mean of frames t-29..t is -10 + 0.2 k with k = 44 - t frames of -4,
    #    first below -9.5 at t = 42 (k = 2: -9.6; t = 41: -9.4)
    bounds[3] = (10, 50, 75)
    frames[:, 3] = -10.0
    frames[:15, 3] = -4.0
    # 4: runs to its bound
    bounds[4] = (5, 10, 50)
    p[:, 4] = 0.1
    # 5: never fires inside the window
    bounds[5] = (5, 10, 200)
    p[:, 5] = 0.1
    logits = torch.log(p / (1 - p))
    want = _ref_stop_rule(frames, logits, bounds, thr, post, steps)
    assert want == [11, 21, 46, 43, 50, 0], want

    L1 = steps + 1
    SENT = 123.0
    mel = torch.full((B, L1, M), SENT, device="cuda")
    mel[:, 0] = 0.0
    stop_all = torch.full((steps, B), SENT, device="cuda")
    t_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    live = torch.full((1,), B, dtype=torch.int32, device="cuda")
    rb = torch.tensor([[r[k] for r in bounds] for k in range(3)], dtype=torch.int32, device="cuda")
    fo, st = torch.empty(B, M, device="cuda"), torch.empty(B, device="cuda")
    fr_d, lg_d = frames.cuda(), logits.cuda()
    for t in range(steps):
        fo.copy_(fr_d[t])
        st.copy_(lg_d[t])
        kk.call("kk_decode_epilogue_rows", fo, st, mel, stop_all, t_dev, done, nfr, live, rb[0], rb[1], rb[2], B, L1, M, thr, post)
    torch.cuda.synchronize()
    assert int(t_dev.item()) == steps
    assert nfr.cpu().tolist() == want
    assert done.cpu().tolist() == [1 if w else 0 for w in want]
    assert int(live.item()) == sum(1 for w in want if w == 0)
    ref_mel = torch.full((B, L1, M), SENT)
    ref_mel[:, 0] = 0.0
    ref_stop = torch.full((steps, B), SENT)
    for b in range(B):
        n = want[b] or steps
        ref_mel[b, 1:n + 1] = frames[:n, b]
        ref_stop[:n, b] = logits[:n, b]
    assert torch.equal(mel.cpu(), ref_mel), "a finished row is never written again"
    assert torch.equal(stop_all.cpu(), ref_stop)
