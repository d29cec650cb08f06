"""The denoising kernels (csrc/kk_denoise.hip) through the C ABI against the fp64 restatement (kokoro_ruslan_amd.denoise_torch).

Bound: relative L2 <= 1e-5 over each whole waveform and over its first and last 768 samples alone, the bound the fp32 STFT / iSTFT
kernels of tests/test_griffinlim_kernels_gpu.py are held to (the gain is continuous in the magnitude: no conditioning of its own).
Bias 0.05 (1 + cos(k / 20)): some bins are gated to zero and others are not; strengths 0.005, 1 and 50 (most bins clamp).
Waveforms: seeded noise plus two sinusoids at 1024 samples (the minimum: every frame touches the reflect padding), 1279 and 1280
(either side of a frame-count step, a tail shorter than a hop), one hop and 57 samples past a tile (one frame in the second tile), three
tiles with a ragged tail, and 22050.  Packed in two orders, every output is bit for bit the output of the waveform alone."""
import math

import pytest
import torch

from kokoro_ruslan_amd import denoise_torch as DT
from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.griffinlim import HOP, N_BINS, hann_window, twiddles

pytestmark = pytest.mark.gpu
STRENGTHS = [0.005, 1.0, 50.0]
TOL, EDGE = 1e-5, 768
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tile():
    return int(kk.load().kk_denoise_tile_frames())


def _lengths():
    t = _tile()
    return [1024, 1279, 1280, HOP * t + 57, HOP * (2 * t + 3) + 100, 22050]


def _bias():
    return (0.05 * (1.0 + torch.cos(torch.arange(N_BINS, dtype=torch.float64) / 20.0))).float()


def _wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    x = 0.005 * torch.randn(n, dtype=torch.float64, generator=g)
    x = x + 0.5 * torch.sin(2 * math.pi * 440.0 * t / 22050) + 0.3 * torch.sin(2 * math.pi * 3100.0 * t / 22050 + 1.0)
    return x.float()


def _waves():
    if "waves" not in _cache:
        _cache["waves"] = [_wave(n, seed=10 + i) for i, n in enumerate(_lengths())]
    return _cache["waves"]


def _f32(s):
    return float(torch.tensor(s, dtype=torch.float32))              # the strength the kernel sees


def _oracle(i, s):
    if ("ref", i, s) not in _cache:
        _cache["ref", i, s] = DT.denoise(_waves()[i], _bias(), _f32(s))
    return _cache["ref", i, s]


def _tables():
    if "tables" not in _cache:
        _cache["tables"] = (torch.view_as_real(twiddles()).contiguous().cuda(), hann_window(torch.float64).float().cuda())
    return _cache["tables"]


def _run(waves, s):
    """kk_denoise on the waveforms packed back to back: the outputs, split."""
    tw, win = _tables()
    n = [int(w.numel()) for w in waves]
    x = torch.cat(waves).contiguous().cuda()
    woff = torch.tensor([0] + n, dtype=torch.int64).cumsum(0).cuda()
    tiles = torch.tensor([[b, f0] for b, m in enumerate(n) for f0 in range(0, -(-m // HOP), _tile())], dtype=torch.int32).cuda()
    y = torch.full_like(x, float("nan"))
    kk.call("kk_denoise", x, woff, tiles, tiles.shape[0], _bias().cuda(), s, tw, win, y)
    return [o.cpu() for o in y.split(n)]


def _alone(i, s):
    if ("alone", i, s) not in _cache:
        _cache["alone", i, s] = _run([_waves()[i]], s)[0]
    return _cache["alone", i, s]


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def test_the_lengths_are_the_edge_cases():
    t = _tile()
    n = _lengths()
    hops = [-(-m // HOP) for m in n]
    assert hops[3] == t + 1 and 1 + n[3] // HOP == t + 1, "one frame (and 57 samples) in the second tile"
    assert hops[4] > 2 * t and n[4] % HOP, "three tiles, ragged tail"
    assert 1 + 1279 // HOP == 5 and 1 + 1280 // HOP == 6


@pytest.mark.parametrize("s", STRENGTHS)
@pytest.mark.parametrize("i", range(6))
def test_denoise_matches_fp64(i, s):
    _need_gpu()
    got, want = _alone(i, s), _oracle(i, s)
    assert got.dtype == torch.float32 and got.shape == want.shape == _waves()[i].shape
    assert bool(torch.isfinite(got).all())
    errs = (_rel(got, want), _rel(got[:EDGE], want[:EDGE]), _rel(got[-EDGE:], want[-EDGE:]))
    print(f"n={got.numel()} s={s}: rel L2 whole {errs[0]:.3e} first {errs[1]:.3e} last {errs[2]:.3e} "
          f"(energy kept {float(want.norm() / _waves()[i].double().norm()):.3f})")
    assert max(errs) <= TOL, (got.numel(), s, errs)


def test_the_gain_gates_some_bins_and_not_others():
    """The cases do what the bound is about: at strength 1 part of the spectrum clamps to zero, at 50 most of it does."""
    w = hann_window(torch.float64)
    from kokoro_ruslan_amd.griffinlim_torch import stft
    M = stft(_waves()[5].double(), w).abs()
    zero = [float((DT.gain(M, _bias(), _f32(s)) == 0).double().mean()) for s in STRENGTHS]
    assert zero[0] < 0.01 and 0.01 < zero[1] < 0.5 and zero[2] > 0.5, zero


@pytest.mark.parametrize("s", [0.005, 1.0])
def test_batch_invariance_bit_for_bit(s):
    _need_gpu()
    waves = _waves()
    for order in ([0, 1, 2, 3, 4, 5], [4, 2, 5, 0, 3, 1]):
        outs = _run([waves[i] for i in order], s)
        for o, i in zip(outs, order):
            assert torch.equal(o, _alone(i, s)), (s, order, i)


def test_stft_mag_mean_matches_fp64():
    _need_gpu()
    tw, win = _tables()
    x = _wave(88 * HOP, seed=3)
    out = torch.full((N_BINS,), float("nan"), device="cuda")
    fr = DT.bias_frames(x.numel())
    kk.call("kk_stft_mag_mean", x.cuda(), x.numel(), fr.start, fr.stop, tw, win, out)
    want = DT.bias_from_wave(x)
    print(f"stft_mag_mean rel L2 {_rel(out.cpu(), want):.3e}")
    assert _rel(out.cpu(), want) <= TOL, _rel(out.cpu(), want)


def test_entry_points_refuse_bad_arguments():
    _need_gpu()
    tw, win = _tables()
    x = torch.zeros(2048, device="cuda")
    woff = torch.tensor([0, 2048], dtype=torch.int64).cuda()
    tiles = torch.tensor([[0, 0]], dtype=torch.int32).cuda()
    b = _bias().cuda()
    with pytest.raises(RuntimeError, match="out != wave"):
        kk.call("kk_denoise", x, woff, tiles, 1, b, 0.1, tw, win, x)
    with pytest.raises(RuntimeError, match="strength"):
        kk.call("kk_denoise", x, woff, tiles, 1, b, -1.0, tw, win, torch.empty_like(x))
    out = torch.empty(N_BINS, device="cuda")
    with pytest.raises(RuntimeError, match="samples"):
        kk.call("kk_stft_mag_mean", x, 1000, 0, 1, tw, win, out)
    with pytest.raises(RuntimeError, match="frames"):
        kk.call("kk_stft_mag_mean", x, 2048, 2, 10, tw, win, out)
