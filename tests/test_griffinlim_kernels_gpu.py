"""Each Griffin-Lim kernel (csrc/kk_griffinlim.hip) against the fp64 torch restatement on a packed ragged batch of 4, 5, 7, 64 and 1003
frames: the shortest utterances are all edge (the window-square envelope varies and the STFT reflects in their first and last three
frames), and 1003 frames make tiles whose last one holds a single frame.

Bounds (relative L2): init <= 1e-6 on the power spectrum S^2 (3e-4 on S, as fp32 torch), one fused iteration <= 1e-5 (also over each utterance's first and last three frames alone), final
iSTFT <= 1e-5."""
import pytest
import torch

from kokoro_ruslan_amd import griffinlim_torch as GT
from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.griffinlim import N_BINS, GriffinLimVocoder

pytestmark = pytest.mark.gpu
FRAMES = [4, 5, 7, 64, 1003]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    return float((a.to(torch.complex128 if a.is_complex() else torch.float64) - b).abs().norm() / b.abs().norm())


def _mels(seed=0):
    return [GT.harmonic_logmel(f, seed=seed + i, f0=100.0 + 20 * i).float() for i, f in enumerate(FRAMES)]


def _state(seed):
    """A mid-iteration state: spectra S . unit phases and a 'previous rebuilt', per utterance [T, 513] complex64."""
    g = torch.Generator().manual_seed(seed)
    S = [GT.magnitude(m.double()).t() for m in _mels(seed)]
    ph = [torch.rand(s.shape, generator=g, dtype=torch.float64) * 6.283185307179586 for s in S]
    Y = [(s * torch.polar(torch.ones_like(p), p)).to(torch.complex64) for s, p in zip(S, ph)]
    R = [(torch.randn(s.shape, generator=g, dtype=torch.float64) * s).to(torch.complex64) for s in S]
    return [s.float() for s in S], Y, R


def _cat(xs):
    return torch.cat(xs).contiguous().cuda()


def test_init_matches_fp64():
    _need_gpu()
    voc = GriffinLimVocoder()
    mels = _mels()
    g = torch.Generator().manual_seed(3)
    ang = [torch.rand((f, N_BINS), dtype=torch.complex64, generator=g) for f in FRAMES]
    T = sum(FRAMES)
    S = torch.empty(T, N_BINS, device="cuda")
    Y = torch.empty(T, N_BINS, dtype=torch.complex64, device="cuda")
    R = torch.full((T, N_BINS), float("nan"), dtype=torch.complex64, device="cuda")
    kk.call("kk_gl_init", _cat(mels), T, voc.pinv, torch.view_as_real(_cat(ang)), S, torch.view_as_real(Y), torch.view_as_real(R))
    ref = torch.cat([GT.magnitude(m.double()).t() for m in mels])
    assert _rel(S.cpu() ** 2, ref ** 2) <= 1e-6, _rel(S.cpu() ** 2, ref ** 2)          # the power spectrum P = S^2
    # S = P^(1/2) magnifies fp32 rounding where P ~ 0 (bin 0, bins above 371); the reference's fp32 S is as far from fp64
    ref32 = torch.cat([GT.magnitude(m.float(), torch.float32, solver="gels").t() for m in mels])
    assert _rel(S.cpu(), ref) <= 3e-4 and _rel(ref32, ref) <= 3e-4, (_rel(S.cpu(), ref), _rel(ref32, ref))
    assert _rel(Y.cpu(), S.cpu().double() * torch.cat(ang).to(torch.complex128)) <= 1e-7
    assert torch.equal(R.cpu(), torch.zeros_like(R.cpu()))
    kk.call("kk_gl_init", _cat(mels), T, voc.pinv, None, S, torch.view_as_real(Y), torch.view_as_real(R))     # init "ones"
    assert torch.equal(Y.real.cpu(), S.cpu()) and torch.equal(Y.imag.cpu(), torch.zeros_like(S.cpu()))


@pytest.mark.parametrize("momentum", [0.99, 0.0])
def test_one_fused_iteration_matches_fp64(momentum):
    _need_gpu()
    voc = GriffinLimVocoder()
    S, Y, R = _state(5)
    tiles = voc.tiles(FRAMES).cuda()
    Yin, Rd, Sd = _cat(Y), _cat(R), _cat(S)
    Yout = torch.full_like(Yin, float("nan"))
    beta = momentum / (1 + momentum) if momentum else 0.0
    kk.call("kk_gl_iter", torch.view_as_real(Yin), torch.view_as_real(Yout), torch.view_as_real(Rd), Sd, tiles, tiles.shape[0], voc.tw,
            voc.window, beta)
    w = torch.hann_window(1024, dtype=torch.float64)
    got_y, got_r = Yout.cpu().split(FRAMES), Rd.cpu().split(FRAMES)
    for b, f in enumerate(FRAMES):
        X = GT.stft(GT.istft(Y[b].to(torch.complex128).t(), w), w).t()
        c = X - torch.tensor(beta, dtype=torch.float32).double() * R[b].to(torch.complex128) if momentum else X
        want = S[b].double() * c / (c.abs() + 1e-16)
        assert _rel(got_r[b], X) <= 1e-5, (b, f, _rel(got_r[b], X))
        assert _rel(got_y[b], want) <= 1e-5, (b, f, _rel(got_y[b], want))
        for sl in (slice(0, 3), slice(f - 3, f)):
            assert _rel(got_r[b][sl], X[sl]) <= 1e-5, (b, f, sl, _rel(got_r[b][sl], X[sl]))
            assert _rel(got_y[b][sl], want[sl]) <= 1e-5, (b, f, sl)


def test_final_istft_matches_fp64():
    _need_gpu()
    voc = GriffinLimVocoder()
    _, Y, _ = _state(9)
    tiles = voc.tiles(FRAMES).cuda()
    wave = torch.full((256 * (sum(FRAMES) - len(FRAMES)),), float("nan"), device="cuda")
    kk.call("kk_gl_istft", torch.view_as_real(_cat(Y)), tiles, tiles.shape[0], voc.tw, voc.window, wave)
    w = torch.hann_window(1024, dtype=torch.float64)
    for b, (got, f) in enumerate(zip(wave.cpu().split([256 * (f - 1) for f in FRAMES]), FRAMES)):
        want = GT.istft(Y[b].to(torch.complex128).t(), w)
        assert got.shape == want.shape == (256 * (f - 1),)
        assert _rel(got, want) <= 1e-5, (b, f, _rel(got, want))
        edge = 768
        assert _rel(got[:edge], want[:edge]) <= 1e-5 and _rel(got[-edge:], want[-edge:]) <= 1e-5, (b, f)


def test_iter_rejects_aliased_spectra():
    _need_gpu()
    voc = GriffinLimVocoder()
    Y = torch.zeros(8, N_BINS, 2, device="cuda")
    tiles = voc.tiles([8]).cuda()
    with pytest.raises(RuntimeError, match="y_in != y_out"):
        kk.call("kk_gl_iter", Y, Y, torch.zeros_like(Y), torch.zeros(8, N_BINS, device="cuda"), tiles, 1, voc.tw, voc.window, 0.5)
