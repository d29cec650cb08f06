"""Each vocoder kernel (csrc/kk_vocoder.hip) against an fp64 torch computation on a packed ragged batch whose utterances include
1, 2 and 3 frames: at stage 1 those are shorter than the 25-sample padding of k = 11, d = 5, so taps run past both ends.

Bounds (relative L2): f32 mode <= 1e-5 against fp64; bf16 mode <= 1e-3 against fp64 on the same bf16-rounded operands, and <= 1e-2
against unrounded fp64."""
import pytest
import torch
import torch.nn.functional as F

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.vocoder import pack_conv, pack_convt

pytestmark = pytest.mark.gpu
FRAMES = [1, 2, 3, 6]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def _batch(mult, C, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [f * mult for f in FRAMES]
    x = torch.randn(sum(lens), C, generator=g)
    seg = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    return x, lens, seg


def _ref_rows(x, lens, fn, slope, bf):
    """fn applied to each utterance alone ([C, L] fp64 -> [N, L']), concatenated channels-last."""
    out, s = [], 0
    for L in lens:
        xb = F.leaky_relu(x[s:s + L].double(), slope) if slope != 1.0 else x[s:s + L].double()
        if bf:
            xb = xb.to(torch.bfloat16).double()
        out.append(fn(xb.t()[None])[0].t())
        s += L
    return torch.cat(out)


def _modes():
    return [("f32", 0, 1e-5), ("bf16", 1, 1e-3)]


@pytest.mark.parametrize("C,mult", [(256, 8), (128, 64), (64, 128), (32, 256)])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_conv1d_every_v1_shape(C, mult, k, d):
    _need_gpu()
    x, lens, seg = _batch(mult, C, seed=C + k * 7 + d)
    g = torch.Generator().manual_seed(k * 100 + d)
    w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    R = x.shape[0]
    for mode, bf, tol in _modes():
        dt = torch.bfloat16 if bf else torch.float32
        P = pack_conv(w, dt).cuda()
        y = torch.empty(R, C, device="cuda")
        kk.call("kk_voc_conv1d", x.cuda(), R, C, P, P.shape[2], P.shape[1], b.cuda(), y, C, k, d, 0.1, seg.cuda(), len(lens), None, None,
                0, bf)
        wr = w.double().to(dt).double() if bf else w.double()
        ref = _ref_rows(x, lens, lambda t: F.conv1d(t, wr, b.double(), dilation=d, padding=(k - 1) // 2 * d), 0.1, bf)
        assert float(ref.std()) > 0.05
        assert _rel(y.cpu(), ref) <= tol, (mode, _rel(y.cpu(), ref))
        if bf:
            raw = _ref_rows(x, lens, lambda t: F.conv1d(t, w.double(), b.double(), dilation=d, padding=(k - 1) // 2 * d), 0.1, False)
            assert _rel(y.cpu(), raw) <= 1e-2


@pytest.mark.parametrize("k,u,cin", [(16, 8, 512), (16, 8, 256), (4, 2, 128), (4, 2, 64), (8, 4, 64)])
def test_convtranspose1d_polyphase(k, u, cin):
    _need_gpu()
    cout = cin // 2
    x, lens, seg = _batch(1, cin, seed=k + u + cin)
    g = torch.Generator().manual_seed(k * u)
    w = torch.randn(cin, cout, k, generator=g) * (u / (cin * k)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    R = x.shape[0]
    for mode, bf, tol in _modes():
        dt = torch.bfloat16 if bf else torch.float32
        P = pack_convt(w, u, dt).cuda()
        y = torch.empty(R * u, cout, device="cuda")
        kk.call("kk_voc_convt1d", x.cuda(), R, cin, P, P.shape[2], P.shape[1], b.cuda(), y, cout, k, u, 0.1, seg.cuda(), len(lens), bf)
        wr = w.double().to(dt).double() if bf else w.double()
        ref = _ref_rows(x, lens, lambda t: F.conv_transpose1d(t, wr, b.double(), stride=u, padding=(k - u) // 2), 0.1, bf)
        assert ref.shape == (R * u, cout) and float(ref.std()) > 0.05
        assert _rel(y.cpu(), ref) <= tol, (mode, _rel(y.cpu(), ref))


def test_convtranspose1d_refuses_unsupported_pairs():
    _need_gpu()
    x = torch.zeros(4, 8, device="cuda")
    seg = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    P = torch.zeros(4, 64, 32, device="cuda")
    y = torch.zeros(64, device="cuda")
    for k, u in ((7, 4), (2, 4)):
        with pytest.raises(RuntimeError, match="k - stride even"):
            kk.call("kk_voc_convt1d", x, 4, 8, P, 32, 64, None, y, 4, k, u, 0.1, seg, 1, 0)
    assert kk.load().kk_voc_convt_taps(7, 4, None) == 0


def test_conv_pre():
    _need_gpu()
    x, lens, seg = _batch(1, 80, seed=11)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(512, 80, 7, generator=g) / (80 * 7) ** 0.5
    b = 0.1 * torch.randn(512, generator=g)
    R = x.shape[0]
    for mode, bf, tol in _modes():
        dt = torch.bfloat16 if bf else torch.float32
        P = pack_conv(w, dt).cuda()
        y = torch.empty(R, 512, device="cuda")
        kk.call("kk_voc_conv1d", x.cuda(), R, 80, P, P.shape[2], P.shape[1], b.cuda(), y, 512, 7, 1, 1.0, seg.cuda(), len(lens), None,
                None, 0, bf)
        wr = w.double().to(dt).double() if bf else w.double()
        ref = _ref_rows(x, lens, lambda t: F.conv1d(t, wr, b.double(), padding=3), 1.0, bf)
        assert _rel(y.cpu(), ref) <= tol, (mode, _rel(y.cpu(), ref))


@pytest.mark.parametrize("C", [32, 8])
def test_conv_post_tanh(C):
    _need_gpu()
    x, lens, seg = _batch(256, C, seed=C)
    g = torch.Generator().manual_seed(C)
    w = torch.randn(1, C, 7, generator=g) / (C * 7) ** 0.5
    b = 0.1 * torch.randn(1, generator=g)
    R = x.shape[0]
    y = torch.empty(R, device="cuda")
    kk.call("kk_voc_post", x.cuda(), R, C, w[0].t().contiguous().cuda(), b.cuda(), y, 7, 0.01, seg.cuda(), len(lens))
    ref = _ref_rows(x, lens, lambda t: torch.tanh(F.conv1d(t, w.double(), b.double(), padding=3)), 0.01, False)[:, 0]
    assert float(ref.std()) > 0.05
    assert _rel(y.cpu(), ref) <= 1e-5


@pytest.mark.parametrize("variant", ["residual", "mrf_first", "mrf_accumulate", "mrf_last"])
def test_epilogue_variants(variant):
    _need_gpu()
    C, k, d, nk = 64, 7, 3, 3
    x, lens, seg = _batch(128, C, seed=3)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    res, acc = torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)
    R = x.shape[0]
    for mode, bf, tol in _modes():
        dt = torch.bfloat16 if bf else torch.float32
        P = pack_conv(w, dt).cuda()
        wr = w.double().to(dt).double() if bf else w.double()
        conv = _ref_rows(x, lens, lambda t: F.conv1d(t, wr, b.double(), dilation=d, padding=(k - 1) // 2 * d), 0.1, bf)
        r_in = res.cuda()
        y = acc.clone().cuda()                       # the MRF sum is updated in place, the residual read from its own buffer
        if variant == "residual":
            h = res.clone().cuda()                   # in place: y aliases the residual
            kk.call("kk_voc_conv1d", x.cuda(), R, C, P, P.shape[2], P.shape[1], b.cuda(), h, C, k, d, 0.1, seg.cuda(), len(lens), h, None,
                    0, bf)
            got, ref = h, conv + res.double()
        elif variant == "mrf_first":
            kk.call("kk_voc_conv1d", x.cuda(), R, C, P, P.shape[2], P.shape[1], b.cuda(), y, C, k, d, 0.1, seg.cuda(), len(lens), r_in,
                    None, 0, bf)
            got, ref = y, conv + res.double()
        elif variant == "mrf_accumulate":
            kk.call("kk_voc_conv1d", x.cuda(), R, C, P, P.shape[2], P.shape[1], b.cuda(), y, C, k, d, 0.1, seg.cuda(), len(lens), r_in,
                    y, 0, bf)
            got, ref = y, acc.double() + (conv + res.double())
        else:
            kk.call("kk_voc_conv1d", x.cuda(), R, C, P, P.shape[2], P.shape[1], b.cuda(), y, C, k, d, 0.1, seg.cuda(), len(lens), r_in,
                    y, nk, bf)
            got, ref = y, (acc.double() + (conv + res.double())) / nk
        assert _rel(got.cpu(), ref) <= tol, (variant, mode, _rel(got.cpu(), ref))
