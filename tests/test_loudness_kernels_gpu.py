"""The kernels of csrc/kk_loudness.hip through LoudnessNormaliser against the fp64 oracle (kokoro_ruslan_amd.loudness_torch): seeded
mixtures of tones, noise and silences at the lengths where the block count changes (22050 Hz: N = 8820, S = 2205), one of three seconds
with an odd length, a peak-limited one, and two short ones at rates where N is not 4 S.  Every input is run alone and in one batch in
two orders, with and without the trim.

The bound on L is 0.01 LU: a tenth of the +-0.1 LU meter tolerance of EBU Tech 3341.  The gain follows L, so its relative bound is
10^(0.01 / 20) - 1 = 1.2e-3.  start, end and the gating decisions can only be compared where the oracle's own decision is not on the
edge: every input must have a decision margin of at least 0.01 dB (trim) and 0.01 LU (both gates), which the first test asserts for
every input and which needs no GPU."""
import math

import pytest
import torch

from kokoro_ruslan_amd import loudness_torch as LT

FS = 22050
TARGET, PEAK_DB, TOP_DB = -23.0, -1.0, 40.0
TOL_LU, MIN_MARGIN = 0.01, 0.01
TOL_GAIN = 10 ** (TOL_LU / 20) - 1
LENGTHS = [1, 1023, 8819, 8820, 11024, 11025, 66151]
TRIMS = [None, TOP_DB]
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def make_wave(n: int, seed: int, fs: int = FS, click: bool = False) -> torch.Tensor:
    """fp32 [n]: quiet noise | tone + noise, swelling | digital silence | a softer tone | quiet noise, in fixed proportions of n."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / fs
    noise = torch.randn(n, generator=g, dtype=torch.float64)
    f1, f2 = 180.0 + 40.0 * (seed % 5), 1300.0 + 170.0 * (seed % 7)
    tone = 0.25 * torch.sin(2 * math.pi * f1 * t) + 0.08 * torch.sin(2 * math.pi * f2 * t + 1.0)
    x = torch.zeros(n, dtype=torch.float64)
    a, b, c, d = int(0.14 * n), int(0.55 * n), int(0.63 * n), int(0.88 * n)
    x[:a] = 2e-5 * noise[:a]
    x[a:b] = (tone[a:b] + 0.02 * noise[a:b]) * (0.6 + 0.4 * torch.sin(2 * math.pi * 1.3 * t[a:b]) ** 2)
    x[c:d] = 0.04 * tone[c:d] + 0.001 * noise[c:d]                 # 28 dB down: under the relative gate where the blocks fall in it
    x[d:] = 2e-5 * noise[d:]
    if click:
        x *= 0.05
        x[n // 3] = 0.97
    return x.to(torch.float32)


def inputs():
    if "in" not in _cache:
        d = {f"n{n}": make_wave(n, 100 + i) for i, n in enumerate(LENGTHS)}
        d["click"] = make_wave(11025 + 2 * 2205 + 7, 200, click=True)
        _cache["in"] = d
    return _cache["in"]


def oracle(name: str, trim):
    key = ("or", name, trim)
    if key not in _cache:
        _cache[key] = LT.normalise(inputs()[name], TARGET, PEAK_DB, trim=trim, fs=FS)
    return _cache[key]


def normaliser(fs: int = FS):
    from kokoro_ruslan_amd.loudness import LoudnessNormaliser
    if ("dev", fs) not in _cache:
        _cache[("dev", fs)] = LoudnessNormaliser(sample_rate=fs)
    return _cache[("dev", fs)]


def alone(name: str, trim):
    key = ("alone", name, trim)
    if key not in _cache:
        y, info = normaliser().normalise([inputs()[name].cuda()], TARGET, PEAK_DB, trim_db=trim)
        _cache[key] = (y[0].clone(), info[0])
    return _cache[key]


def test_every_input_is_away_from_the_decision_edges():
    seen = {"blocks": set(), "limited": 0, "silent": 0, "cut": 0}
    for name, x in inputs().items():
        for trim in TRIMS:
            _, info = oracle(name, trim)
            assert info["trim_margin"] >= MIN_MARGIN, (name, trim, info)
            assert info["gate_margin"] >= MIN_MARGIN, (name, trim, info)
            n = info["end"] - info["start"]
            seen["blocks"].add(max(0, (n - 8820) // 2205 + 1) if n >= 8820 else 0)
            seen["limited"] += info["limited"]
            seen["silent"] += info["measured"] is None
        if LT.trim_edges(x, TOP_DB, fs=FS)[:2] != (0, x.numel()):
            seen["cut"] += 1
    assert {0, 1, 2} <= seen["blocks"] and seen["limited"] >= 1 and seen["silent"] >= 3 and seen["cut"] >= 3, seen
    L, margin = LT.integrated_loudness(inputs()["n66151"], FS)     # the relative gate drops blocks of this one
    y = LT.kweight(inputs()["n66151"], FS)
    ungated = -0.691 + 10 * math.log10(float((y.unfold(0, 8820, 2205) ** 2).mean(dim=1).mean()))
    assert L - ungated > 0.5 and margin >= MIN_MARGIN


@pytest.mark.gpu
@pytest.mark.parametrize("trim", TRIMS, ids=["whole", "trimmed"])
def test_alone_matches_the_oracle(trim):
    _need_gpu()
    worst_L = worst_g = 0.0
    for name, x in inputs().items():
        want_y, want = oracle(name, trim)
        got_y, got = alone(name, trim)
        assert (got["start"], got["end"]) == (want["start"], want["end"]), (name, got, want)
        assert got_y.dtype == torch.float32 and got_y.shape == (want["end"] - want["start"],)
        g32 = torch.tensor(got["gain"], dtype=torch.float32)
        assert float(g32) == got["gain"], "the gain reported is the fp32 value applied"
        assert torch.equal(got_y.cpu(), x[want["start"]:want["end"]] * g32), f"{name}: the output is x[start:end] * gain in fp32"
        assert got["limited"] == want["limited"], (name, got, want)
        if want["measured"] is None:
            assert got["measured"] is None and got["gain"] == 1.0 and not got["limited"], (name, got)
            continue
        dL, dg = abs(got["measured"] - want["measured"]), abs(got["gain"] / want["gain"] - 1.0)
        worst_L, worst_g = max(worst_L, dL), max(worst_g, dg)
        assert dL <= TOL_LU, (name, got, want)
        assert dg <= TOL_GAIN, (name, got, want)
        if want["limited"]:
            assert float(got_y.abs().max()) <= 10 ** (PEAK_DB / 20) * (1 + 2.0 ** -23), "the peak ceiling holds"
    print(f"trim {trim}: largest |L_device - L_oracle| {worst_L:.3e} LU, largest relative gain difference {worst_g:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("trim", TRIMS, ids=["whole", "trimmed"])
def test_batch_in_two_orders_is_bit_identical_to_alone(trim):
    _need_gpu()
    names = list(inputs())
    for order in (names, names[::-1][2:] + names[::-1][:2]):
        ys, infos = normaliser().normalise([inputs()[k].cuda() for k in order], TARGET, PEAK_DB, trim_db=trim)
        for k, y, info in zip(order, ys, infos):
            want_y, want = alone(k, trim)
            assert info == want, (k, info, want)                   # floats compared exactly: the same bits
            assert torch.equal(y, want_y), k
    whole = normaliser().measure([inputs()[k].cuda() for k in names])
    assert whole == [alone(k, None)[1]["measured"] for k in names]
    edges = normaliser().trim_edges([inputs()[k].cuda() for k in names], TOP_DB)
    assert edges == [(alone(k, TOP_DB)[1]["start"], alone(k, TOP_DB)[1]["end"]) for k in names]


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [8046, 11025])
def test_rates_where_the_block_is_not_four_steps(fs):
    """N - 4 S is -2 at 8046 Hz and +2 at 11025 Hz: lengths of exactly one, two and three blocks and one sample less."""
    _need_gpu()
    N, S = LT.block_sizes(fs)
    assert N - 4 * S == (-2 if fs == 8046 else 2)
    waves = [make_wave(n, 300 + i, fs) for i, n in enumerate((N - 1, N, N + S - 1, N + S, N + 2 * S, 3 * N + 11))]
    got = normaliser(fs).measure([w.cuda() for w in waves])
    for w, g in zip(waves, got):
        L, margin = LT.integrated_loudness(w, fs)
        assert margin >= MIN_MARGIN, (fs, w.numel(), margin)
        if L == -math.inf:
            assert g is None
        else:
            print(f"fs {fs} n {w.numel()}: |L_device - L_oracle| {abs(g - L):.3e} LU")
            assert abs(g - L) <= TOL_LU, (fs, w.numel(), g, L)
