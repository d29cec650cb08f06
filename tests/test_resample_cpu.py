"""CPU suite for the resampler's contract (kokoro_ruslan_amd.resample_torch) and the host side of the speed perturbation
(kokoro.data.augment): output lengths, the identity, a tone that moves where it should, integer-phase fp32 against fp64, the duration
rescale against the reference's statements (data/dataset.py:755-768), the draws, and load_wav / load_wav_any."""
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import resample_torch as RT


def _signal(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050
    return (0.5 * torch.sin(2 * math.pi * 220 * t) + 0.3 * torch.sin(2 * math.pi * 3100 * t)
            + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()


@pytest.mark.parametrize("orig,new", [(22050, 19845), (22050, 24255), (22050, 20947), (22050, 22793), (44100, 22050), (48000, 22050),
                                      (16000, 22050)])
@pytest.mark.parametrize("L", [1, 700, 3001])
def test_length_is_ceil(orig, new, L):
    y = RT.resample(_signal(L), orig, new)
    assert y.shape == (math.ceil(new * L / orig),) == (RT.resampled_length(L, orig, new),)
    assert y.dtype == torch.float64 and bool(torch.isfinite(y).all())


def test_rate_pairs():
    assert RT.rate_pair(22050, 19845)[:2] == (10, 9) and RT.rate_pair(22050, 24255)[:2] == (10, 11)
    assert RT.rate_pair(22050, 20947)[:2] == (22050, 20947)
    assert RT.rate_pair(44100, 22050)[:2] == (2, 1) and RT.rate_pair(44100, 22050)[3] == 13
    assert RT.rate_pair(48000, 22050)[:2] == (320, 147) and RT.rate_pair(48000, 22050)[3] == 14
    assert RT.rate_pair(16000, 22050)[:2] == (320, 441)
    with pytest.raises(ValueError):
        RT.rate_pair(0, 22050)


def test_equal_rates_are_the_identity():
    x = _signal(500)
    assert RT.resample(x, 22050, 22050) is x
    assert torch.equal(RT.resample(x, 22050, int(22050 * 1.00001)), x)


def test_tone_moves_with_the_rate():
    """440 Hz at 22050 Hz, resampled to 24255 Hz and read at 22050 Hz again, is a 400 Hz tone (speed factor 1.1 slows it down)."""
    n = 22050
    x = torch.sin(2 * math.pi * 440 * torch.arange(n, dtype=torch.float64) / 22050)
    y = RT.resample(x, 22050, 24255)
    assert y.shape == (24255,)
    spec = torch.fft.rfft(y[:22050] * torch.hann_window(22050, dtype=torch.float64)).abs()
    assert int(spec.argmax()) == 400                                  # 1 Hz bins
    assert abs(float(y[2000:-2000].abs().max()) - 1.0) < 0.02         # unit gain in the pass band


@pytest.mark.parametrize("new", [19845, 20947, 22793, 22047])
def test_integer_phase_fp32_stays_near_fp64(new):
    x = _signal(12000)
    want = RT.resample(x, 22050, new)
    got = RT.resample(x, 22050, new, dtype=torch.float32)
    assert got.dtype == torch.float32
    rel = float((got.double() - want).norm() / want.norm())
    ta = float((RT.resample(x, 22050, new, dtype=torch.float32, order="torchaudio").double() - want).norm() / want.norm())
    ta64 = float((RT.resample(x, 22050, new, order="torchaudio") - want).norm() / want.norm())
    print(f"22050 -> {new}: integer-phase fp32 {rel:.2e}, torchaudio's order in fp32 {ta:.2e}, in fp64 {ta64:.2e}")
    assert rel <= 1e-6
    assert ta64 <= 1e-10                                              # the two orders are the same function


def test_duration_rescale_restates_the_reference():
    from kokoro.data.augment import rescale_durations
    dur = torch.tensor([5, 7, 3, 12, 1, 0, 0], dtype=torch.long)      # sum 28; 5 / 2 = 2.5 and 7 / 2 = 3.5 round to even; a zero-length tail
    f, T_new = 2.0, 15
    # data/dataset.py:757-768, statement for statement
    scaled = dur.float() / f
    want = torch.clamp(scaled.round().long(), min=1)
    diff = T_new - want.sum().item()
    if diff != 0 and len(want) > 0:
        want[-1] = max(1, want[-1] + diff)
    want = torch.clamp(want, min=1)
    got = rescale_durations(dur, f, T_new, 28)
    assert torch.equal(got, want)
    assert got.tolist() == [2, 4, 2, 6, 1, 1, 1]                      # sum 17 > 15: the clamp keeps the tail at 1
    got = rescale_durations(dur, 0.9, 31, 28)
    assert got.tolist()[:5] == [6, 8, 3, 13, 1] and int(got.sum()) == 33 and got.tolist()[-2:] == [1, 1]
    got = rescale_durations(torch.tensor([5, 7, 3, 12, 1]), 1.1, 25, 28)
    assert got.tolist() == [5, 6, 3, 11, 1]                           # sum 26 for 25 frames: the last phoneme cannot go below 1
    got = rescale_durations(torch.tensor([5, 7, 3, 12, 9]), 1.1, 30, 36)
    assert got.tolist() == [5, 6, 3, 11, 5] and int(got.sum()) == 30  # 9 / 1.1 rounds to 8, the reconcile takes 3 more off the last


def test_unaligned_durations_are_recomputed():
    from kokoro.data.augment import rescale_durations
    from kokoro.data.features import fallback_durations
    cached = fallback_durations(7, 100)
    assert torch.equal(rescale_durations(cached, 1.07, 93, 100), fallback_durations(7, 93))
    aligned = cached.clone()
    aligned[0] += 1
    aligned[1] -= 1
    got = rescale_durations(aligned, 1.07, 93, 100)
    assert not torch.equal(got, fallback_durations(7, 93)) and int(got.sum()) == 93


def test_draws_are_a_pure_function():
    from kokoro.data.augment import draw_factor, mel_frames, perturbed_samples
    a = [draw_factor(0, 3, i, 0.5, 0.1) for i in range(400)]
    assert a == [draw_factor(0, 3, i, 0.5, 0.1) for i in range(400)]
    hit = [f for f in a if f != 1.0]
    assert 140 <= len(hit) <= 260 and all(0.9 <= f <= 1.1 for f in hit)
    assert a != [draw_factor(0, 4, i, 0.5, 0.1) for i in range(400)] and a != [draw_factor(1, 3, i, 0.5, 0.1) for i in range(400)]
    assert all(draw_factor(0, 0, i, 0.0, 0.1) == 1.0 for i in range(50))
    assert all(draw_factor(0, 0, i, 1.0, 0.1) != 1.0 for i in range(50))
    # the reference's order of draws: random() decides, the next uniform() is the factor
    import random
    r = random.Random("kokoro-speed-perturb:0:3:7")
    u = r.random()
    assert draw_factor(0, 3, 7, 1.0, 0.1) == 1.0 + r.uniform(-0.1, 0.1) and (draw_factor(0, 3, 7, 0.5, 0.1) != 1.0) == (u < 0.5)
    for L, f in ((30000, 0.95), (700, 1.0999), (1, 0.9), (77000, 1.0337)):
        assert perturbed_samples(L, f) == RT.resampled_length(L, 22050, int(22050 * f))
    assert mel_frames(700, 1800) == 5 and mel_frames(30000, 1800) == 118 and mel_frames(10 ** 6, 1800) == 1800


def test_perturbation_over_a_dataset(tmp_path):
    """SpeedPerturbation on a two-utterance corpus: lengths from the wav headers, items with rescaled host-side fields."""
    from scipy.io import wavfile
    from kokoro.data.augment import SpeedPerturbation, mel_frames, perturbed_samples
    from kokoro.data.cached import CachedFeatureDataset
    from kokoro.data.features import cache_entry, write_cache_entry
    wavs, cache = tmp_path / "wavs", tmp_path / "cache"
    wavs.mkdir()
    for i, n in enumerate((9000, 14000)):
        a = (_signal(n, seed=i).numpy() * 20000).astype(np.int16)
        wavfile.write(wavs / f"u{i}.wav", 22050, a)
        T = 1 + n // 256
        ft = {"mel_spec": torch.zeros(80, T), "pitch": torch.zeros(T), "energy": torch.zeros(T), "mel_length": T}
        write_cache_entry(cache, cache_entry(ft, f"u{i}", torch.arange(1, 6 + i), None, None if i else torch.tensor([8, 7, 6, 9, 6])))
    ds = CachedFeatureDataset(str(cache))
    sp = SpeedPerturbation(ds, str(wavs), prob=1.0, spread=0.1, seed=0)
    for i in range(2):
        f = sp.factor(i, 0)
        n = (9000, 14000)[i]
        assert sp.wav_length(i) == n and sp.perturbed_length(i, 0) == mel_frames(perturbed_samples(n, f), 1800)
        it = sp.item(i, 0, ds[i])
        a, f2 = it["_perturb"]
        assert f2 == f and a.dtype == np.int16 and a.shape == (n,)
        assert it["mel_length"] == sp.perturbed_length(i, 0) and it["stop_token_targets"].shape == (it["mel_length"],)
        assert float(it["stop_token_targets"][-1]) == 1.0 and int(it["phoneme_durations"].sum()) == it["mel_length"]
        assert it["_np"]["mel"].shape == (it["mel_length"], 80) and not it["_np"]["mel"].any()
    assert SpeedPerturbation(ds, str(wavs), prob=0.0).item(0, 0, ds[0]) is None
    (wavs / "u1.wav").unlink()
    with pytest.raises(FileNotFoundError, match="1 of 2"):
        SpeedPerturbation(ds, str(wavs))


def test_load_wav_any_and_load_wav(tmp_path):
    from scipy.io import wavfile
    from kokoro.data.features import load_wav, load_wav_any
    a = (np.sin(np.arange(1600) * 0.05) * 12000).astype(np.int16)
    wavfile.write(tmp_path / "k16.wav", 16000, a)
    wavfile.write(tmp_path / "k22.wav", 22050, a)
    with pytest.raises(ValueError, match="resampl"):
        load_wav(tmp_path / "k16.wav")
    sr, x = load_wav_any(tmp_path / "k16.wav")
    assert sr == 16000 and x.dtype == torch.float32 and np.array_equal(x.numpy(), a.astype(np.float32) / 32768.0)
    sr, y = load_wav_any(tmp_path / "k22.wav")
    assert sr == 22050 and torch.equal(y, load_wav(tmp_path / "k22.wav"))
