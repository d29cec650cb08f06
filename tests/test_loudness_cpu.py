"""The fp64 loudness oracle (kokoro_ruslan_amd.loudness_torch) against the written definitions: the standard's 48 kHz coefficient
table, sines of known loudness, a gating case, the degenerate inputs, hand-computed trim positions, and normalise's target and peak
ceiling.  No GPU."""
import math

import pytest
import torch

from kokoro_ruslan_amd import loudness_torch as LT


def _sine(fs, seconds, amp=1.0, f=997.0):
    t = torch.arange(int(round(seconds * fs)), dtype=torch.float64) / fs
    return amp * torch.sin(2 * math.pi * f * t)


def test_48k_coefficients_are_the_standards_table():
    (b1, a1), (b2, a2) = LT.kweight_coeffs(48000)
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585]
    for got, w in zip(b1 + a1[1:], want):
        assert abs(got - w) <= 1e-10, (got, w)
    assert a1[0] == a2[0] == 1.0 and b2 == [1.0, -2.0, 1.0]
    assert abs(a2[1] - -1.99004745483398) <= 1e-10 and abs(a2[2] - 0.99007225036621) <= 1e-10


def test_chunked_biquad_is_the_sample_by_sample_recursion():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3001, generator=g, dtype=torch.float64)
    for b, a in LT.kweight_coeffs(22050):
        s1 = s2 = 0.0
        want = []
        for v in x.tolist():
            y = b[0] * v + s1
            s1, s2 = b[1] * v - a[1] * y + s2, b[2] * v - a[2] * y
            want.append(y)
        want = torch.tensor(want, dtype=torch.float64)
        for chunk in (256, 7):
            assert float((LT.biquad(x, b, a, chunk) - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_sine_loudness():
    L48, _ = LT.integrated_loudness(_sine(48000, 5.0), 48000)
    L22, _ = LT.integrated_loudness(_sine(22050, 5.0), 22050)
    print(f"997 Hz sine: {L48:.4f} LUFS at 48 kHz, {L22:.4f} at 22050 Hz")
    assert abs(L48 - -3.010) <= 0.005 and abs(L22 - -2.981) <= 0.005
    for fs, L in ((48000, L48), (22050, L22)):
        quiet, _ = LT.integrated_loudness(_sine(fs, 5.0, 0.1), fs)
        assert abs(quiet - (L - 20.0)) <= 1e-9


def test_gating():
    lo, hi = 10 ** (-36 / 20), 10 ** (-23 / 20)
    x = torch.cat([_sine(22050, 2.0, lo), _sine(22050, 6.0, hi), _sine(22050, 2.0, lo)])
    L, margin = LT.integrated_loudness(x, 22050)
    print(f"gated {L:.4f} LUFS, margin {margin:.3f} LU")
    assert abs(L - -26.182) <= 0.005
    assert margin >= 1.0


def test_no_block_and_silence_measure_none():
    g = torch.Generator().manual_seed(1)
    assert LT.integrated_loudness(torch.randn(8819, generator=g), 22050)[0] == -math.inf
    assert LT.integrated_loudness(torch.randn(8820, generator=g), 22050)[0] > -math.inf
    assert LT.integrated_loudness(torch.zeros(30000), 22050)[0] == -math.inf
    for x in (torch.randn(8819, generator=g), torch.zeros(30000)):
        y, info = LT.normalise(x)
        assert info["measured"] is None and info["gain"] == 1.0 and not info["limited"]
        assert torch.equal(y, x.double())


def test_trim_positions_by_hand():
    fs = 22050
    g = torch.Generator().manual_seed(2)
    a, b, c = 6615, 22050, 4410                                  # 0.3 s of noise at 1e-4 | 1 s tone | 0.2 s of noise at 1e-4
    x = torch.cat([1e-4 * torch.randn(a, generator=g, dtype=torch.float64), _sine(fs, 1.0, 0.5),
                   1e-4 * torch.randn(c, generator=g, dtype=torch.float64)])
    start, end, margin = LT.trim_edges(x, 40.0, 50.0, fs=fs)
    # frame t covers [256 t - 512, 256 t + 512).  The loudest frames lie wholly in the tone (mean square 0.125); a frame with k tone
    # samples has 10 log10(k / 1024) dB (the noise adds 1e-8 per sample: nothing), above -40 dB from k >= 0.1024, i.e. k >= 1.
    first = min(t for t in range(1 + len(x) // 256) if 256 * t + 512 > a + 1)       # (the tone's sample 0 is sin(0) = 0)
    last = max(t for t in range(1 + len(x) // 256) if 256 * t - 512 < a + b)
    m = round(50.0 * fs / 1000)
    assert (first, last, m) == (24, 113, 1102)
    assert (start, end) == (first * 256 - m, (last + 1) * 256 + m) == (5042, 30286)
    assert margin > 0.01
    assert LT.trim_edges(x, 40.0, 0.0, fs=fs)[:2] == (first * 256, (last + 1) * 256)
    assert LT.trim_edges(x, 40.0, 1000.0, fs=fs)[:2] == (0, len(x))             # the margin is clipped to the waveform


def test_all_loud_and_all_zero_are_untrimmed():
    x = _sine(22050, 0.5, 0.3)
    assert LT.trim_edges(x, 40.0, 50.0)[:2] == (0, len(x))
    assert LT.trim_edges(x, 40.0, 0.0)[:2] == (0, len(x))        # frame 0 holds 512 samples of the tone: -3 dB
    assert LT.trim_edges(torch.zeros(5000))[:2] == (0, 5000)
    assert LT.trim_edges(torch.zeros(1))[:2] == (0, 1)


def test_normalise_reaches_the_target():
    g = torch.Generator().manual_seed(3)
    x = 0.05 * torch.randn(40000, generator=g) * (1.0 + _sine(22050, 40000 / 22050, 0.5, 3.0)).float()
    for target in (-23.0, -16.0):
        y, info = LT.normalise(x, target_lufs=target, peak_db=0.0)
        assert not info["limited"] and (info["start"], info["end"]) == (0, 40000)
        assert abs(LT.integrated_loudness(y, 22050)[0] - target) <= 1e-6
        assert abs(info["gain"] - 10 ** ((target - info["measured"]) / 20)) <= 1e-12
    silence = torch.zeros(9000)
    y, info = LT.normalise(torch.cat([silence, x, silence]), trim=40.0)
    assert info["start"] > 0 and info["end"] < 58000 and y.numel() == info["end"] - info["start"]
    assert abs(LT.integrated_loudness(y, 22050)[0] - -23.0) <= 1e-6


def test_peak_ceiling_holds_and_sets_limited():
    x = _sine(22050, 1.0, 0.01)
    x[5000] = 0.9                                                # a click: the gain that reaches -23 LUFS would take it far over full scale
    y, info = LT.normalise(x, target_lufs=-23.0, peak_db=-1.0)
    assert info["limited"] and abs(float(y.abs().max()) - 10 ** (-1 / 20)) <= 1e-12
    assert LT.integrated_loudness(y, 22050)[0] < -23.0
    y, info = LT.normalise(_sine(22050, 1.0, 0.5), target_lufs=-23.0, peak_db=-1.0)
    assert not info["limited"] and float(y.abs().max()) < 10 ** (-1 / 20)


@pytest.mark.parametrize("fs", [8046, 11025, 16000, 44100])
def test_block_sizes_follow_the_rate(fs):
    N, S = LT.block_sizes(fs)
    assert (N, S) == (round(0.4 * fs), round(0.1 * fs)) and abs(N - 4 * S) <= 2
    g = torch.Generator().manual_seed(fs)
    x = 0.1 * torch.randn(N + S - 1, generator=g)                # one whole block, and not yet two
    y = LT.kweight(x, fs)
    assert abs(LT.integrated_loudness(x, fs)[0] - (-0.691 + 10 * math.log10(float((y[:N] ** 2).mean())))) <= 1e-9
