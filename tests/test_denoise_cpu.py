"""The fp64 restatement of spectral denoising (kokoro_ruslan_amd.denoise_torch) against what the method says, and kokoro-synth's --denoise
argument errors, which are decided before anything touches the GPU."""
import math

import pytest
import torch

from kokoro.cli import synth as cli
from kokoro_ruslan_amd import denoise_torch as DT
from kokoro_ruslan_amd.griffinlim import N_BINS, hann_window
from kokoro_ruslan_amd.griffinlim_torch import stft


def _tone(n, k, amp=1.0, phase=0.0):
    """A sinusoid centred on bin k of the 1024-point transform."""
    return amp * torch.sin(2 * math.pi * k * torch.arange(n, dtype=torch.float64) / 1024 + phase)


def _noise(n, seed=0):
    return torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_strength_zero_returns_the_input():
    x = _noise(5000) + _tone(5000, 40)
    b = torch.rand(N_BINS, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    y = DT.denoise(x, b, 0.0)
    assert y.dtype == torch.float64 and y.shape == x.shape
    assert float((y - x).abs().max()) <= 1e-12


def test_a_huge_bias_returns_zeros():
    x = _noise(4096, seed=2)
    y = DT.denoise(x, torch.full((N_BINS,), 1e9, dtype=torch.float64), 1.0)
    assert torch.equal(y, torch.zeros_like(y))


def test_a_one_bin_bias_changes_the_spectrum_only_near_that_bin():
    n, k_hit, k_far = 256 * 40, 100, 300
    x = _tone(n, k_hit) + _tone(n, k_far, amp=0.7, phase=0.3)
    b = torch.zeros(N_BINS, dtype=torch.float64)
    b[k_hit] = 1.0
    w = hann_window(torch.float64)
    X = stft(x, w).abs()
    # frames 0 .. 2 and F - 3 .. F - 1 see the reflect padding, where the tones are not stationary; what the gain changes there reaches
    # the samples below 1024 (above N - 1024), which the windows of frames 6 .. F - 7 do not touch
    interior = slice(6, X.shape[1] - 6)
    s = 0.5 * float(X[k_hit, interior].min())              # half the tone's magnitude in its own bin
    Y = stft(DT.denoise(x, b, s), w).abs()
    d = (Y - X).abs()[:, interior]
    assert float(d[k_hit].min()) > 0.1 * s, "the gated bin moved"
    near = torch.zeros(N_BINS, dtype=torch.bool)
    near[k_hit - 4:k_hit + 5] = True                        # the Hann main lobe and what overlap-add spreads of it
    assert float(d[~near].max()) <= 1e-6 * float(X.max()), float(d[~near].max())
    assert float(Y[k_far, interior].min()) > 0.99 * float(X[k_far, interior].min())


def test_bias_of_a_stationary_sinusoid_peaks_at_its_bin():
    b = DT.bias_from_wave(_tone(88 * 256, 77) + 1e-3 * _noise(88 * 256, seed=3))
    assert b.shape == (N_BINS,) and b.dtype == torch.float64 and int(b.argmax()) == 77
    assert list(DT.bias_frames(88 * 256)) == list(range(2, 87))
    # the mean over the interior frames of a stationary tone is what any one of them shows: amplitude . sum(window) / 2
    assert abs(float(b[77]) - 256.0) <= 1.0


@pytest.mark.parametrize("n", [1024, 1279, 1280, 22050])
def test_length_is_kept(n):
    x = _noise(n, seed=n)
    y = DT.denoise(x, torch.full((N_BINS,), 0.1, dtype=torch.float64), 1.0)
    assert y.shape == (n,) and bool(torch.isfinite(y).all())


def test_short_waveform_is_refused():
    with pytest.raises(ValueError, match="1024"):
        DT.denoise(torch.zeros(1023, dtype=torch.float64), torch.zeros(N_BINS), 0.1)


BASE = ["--checkpoint", "missing.pth", "--ids", "missing.jsonl", "--output", "missing"]


def test_parser_denoise_values():
    p = cli.build_parser()
    assert p.parse_args(BASE).denoise is None
    assert p.parse_args(BASE + ["--vocoder", "v", "--denoise"]).denoise == 0.005
    assert p.parse_args(BASE + ["--vocoder", "v", "--denoise", "0.02"]).denoise == 0.02
    a = p.parse_args(BASE + ["--denoise", "--vocoder", "v"])
    assert a.denoise == 0.005 and a.vocoder == "v"
    cli.check_args(p, a)


@pytest.mark.parametrize("extra", [["--denoise"], ["--denoise", "0.01"], ["--griffin-lim", "--denoise"],
                                   ["--griffin-lim", "--vocoder", "v", "--denoise"], ["--vocoder", "v", "--denoise", "-0.5"],
                                   ["--vocoder", "v", "--denoise", "nan"]])
def test_kokoro_synth_denoise_argument_errors(extra, capsys):
    """parser.error (exit status 2) from main() itself: the checkpoint and the ids file do not exist, so nothing was read."""
    with pytest.raises(SystemExit) as e:
        cli.main(BASE + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--denoise" in err or "--griffin-lim and --vocoder" in err
