"""CPU suite of the feature front-end: features_torch against the reference's recorded pitch and energy (tests/golden/features.npz,
written by tests/golden/make_features_golden.py), stop targets, fallback durations and the reconcile rule against the recorded ones,
load_wav's rules, the cache writer through CachedFeatureDataset and collate_fn, and kokoro-precompute's flag checks.

The 1e-6 on pitch and energy: the reference itself, run in fp32 and in fp64 on eight signals of this family (2278 frames), differs by
at most 7.7e-8 on any frame with no voicing decision changed, so a faithful restatement has more than 10x room and a wrong clamp,
quantile rule or lag range has none."""
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import features_torch as FT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _wave(gold, i):
    return torch.from_numpy(gold[f"signal_{i}"]).float() / 32768.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_matches_the_reference(gold, dtype):
    frames = 0
    for i, n in enumerate(gold["lengths"]):
        w = _wave(gold, i)
        assert w.shape[0] == n
        out = FT.extract(w, dtype=dtype)
        T = 1 + max(int(n), 1024) // 256
        assert out["mel_length"] == T == FT.mel_frames(n) and out["mel_spec"].shape == (80, T) and out["mel_spec"].dtype == dtype
        want_p = torch.from_numpy(gold[f"pitch_{i}"]).double()
        assert out["pitch"].shape == want_p.shape == (T,)
        assert float((out["pitch"].double() - want_p).abs().max()) <= 1e-6, i
        assert bool(((out["pitch"] > 0) == (want_p > 0)).all()), i
        lin64 = FT.mel_linear(FT.normalise(w, torch.float64))
        clip = int(gold["clip"])
        for key, lin in ((f"energy_{i}", lin64), (f"energy_clip_{i}", lin64[:, :clip])):
            e = FT.energy(lin.to(dtype))
            assert float((e.double() - torch.from_numpy(gold[key]).double()).abs().max()) <= 1e-6, key
        frames += T
    assert frames >= 1000


def test_clipping_statistics(gold):
    """max_seq_length cuts mel and energy (statistics over the kept frames); the pitch statistics run over all frames."""
    w = _wave(gold, 4)
    full, cut = FT.extract(w), FT.extract(w, max_seq_length=64)
    assert cut["mel_length"] == 64 and torch.equal(cut["mel_spec"], full["mel_spec"][:, :64])
    assert torch.equal(cut["pitch"], full["pitch"][:64])
    assert float((cut["energy"].double() - torch.from_numpy(gold["energy_clip_4"]).double()).abs().max()) <= 1e-6
    assert not torch.allclose(cut["energy"], full["energy"][:64])


def test_all_zero_and_variance_off(gold):
    z = FT.extract(torch.zeros(5000), dtype=torch.float32)
    assert torch.equal(z["mel_spec"], torch.full((80, 20), 1e-9).log()) and not z["pitch"].any() and not z["energy"].any()
    off = FT.extract(_wave(gold, 2), variance=False)
    assert not off["pitch"].any() and not off["energy"].any() and off["pitch"].shape == (129,)


def test_frame_counts():
    for n in (1, 700, 1023, 1024, 1279, 1280, 3000, 143000):
        assert FT.extract(torch.ones(n), variance=False)["mel_length"] == 1 + max(n, 1024) // 256
        assert FT.pitch_candidates(FT.normalise(torch.ones(n)))[0].shape[0] == 1 + max(n, 2048) // 256 == FT.pitch_frames(n)


def test_stop_targets_fallback_and_reconcile(gold):
    from kokoro.data import features as DF
    from kokoro.data.cached import reference_reconcile
    for T in (0, 1, 3, 5, 6, 64, 301):
        got = DF.stop_token_targets(T)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), gold[f"stop_{T}"]), T
    for P, T in gold["fallback_cases"].tolist():
        got = DF.fallback_durations(P, T)
        assert got.dtype == torch.long and np.array_equal(got.numpy(), gold[f"fallback_{P}_{T}"]), (P, T)
        assert P == 0 or int(got.sum()) == T
    # dataset.py:761-768 on given durations: the last phoneme takes the difference, never below 1, then everything >= 1
    feats = {"mel_spec": torch.zeros(80, 21), "pitch": torch.zeros(21), "energy": torch.zeros(21), "mel_length": 21}
    for dur in ([2] * 8, [5] * 8, [0, 3, 30], [21]):
        e = DF.cache_entry(feats, "u", torch.arange(1, len(dur) + 1), None, torch.tensor(dur))
        assert torch.equal(e["phoneme_durations"], reference_reconcile(torch.tensor(dur), 21))
    assert DF.cache_entry(feats, "u", torch.arange(1, 9), None, torch.tensor([2] * 8))["phoneme_durations"].tolist() == [2] * 7 + [7]
    assert DF.cache_entry(feats, "u", torch.arange(1, 4), None, torch.tensor([0, 3, 30]))["phoneme_durations"].tolist() == [1, 3, 18]
    assert torch.equal(DF.cache_entry(feats, "u", torch.arange(1, 6))["phoneme_durations"], DF.fallback_durations(5, 21))
    with pytest.raises(ValueError, match="phoneme_durations"):
        DF.cache_entry(feats, "u", torch.arange(1, 6), None, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="stress_indices"):
        DF.cache_entry(feats, "u", torch.arange(1, 6), torch.zeros(4, dtype=torch.long))


def test_load_wav_rules(tmp_path):
    from scipy.io import wavfile
    from kokoro.data.features import load_wav
    rng = np.random.default_rng(0)
    a16 = rng.integers(-32768, 32767, 500).astype(np.int16)
    a32 = rng.integers(-2 ** 31, 2 ** 31 - 1, 500).astype(np.int32)
    af = rng.standard_normal(500).astype(np.float32) * 3
    st = rng.integers(-32768, 32767, (500, 2)).astype(np.int16)
    for name, arr in (("a16", a16), ("a32", a32), ("af", af), ("st", st)):
        wavfile.write(str(tmp_path / f"{name}.wav"), 22050, arr)
    assert np.array_equal(load_wav(tmp_path / "a16.wav").numpy(), a16.astype(np.float32) / 32768.0)
    assert np.array_equal(load_wav(tmp_path / "a32.wav").numpy(), a32.astype(np.float32) / 2147483648.0)
    assert np.array_equal(load_wav(tmp_path / "af.wav").numpy(), af)
    want = torch.from_numpy(st.astype(np.float32) / 32768.0).T.mean(dim=0)
    got = load_wav(tmp_path / "st.wav")
    assert got.shape == (500,) and got.dtype == torch.float32 and torch.equal(got, want)
    wavfile.write(str(tmp_path / "sr.wav"), 16000, a16)
    with pytest.raises(ValueError, match="resampl"):
        load_wav(tmp_path / "sr.wav")


def test_cache_entries_load_and_collate(gold, tmp_path):
    from kokoro.data import features as DF
    from kokoro.data.cached import CachedFeatureDataset, collate_fn
    lens = {}
    for i, P in ((1, 4), (2, 9), (3, 30)):
        f = FT.extract(_wave(gold, i), dtype=torch.float32)
        f.pop("mel_linear")
        e = DF.cache_entry(f, f"utt{i}", torch.arange(1, P + 1), torch.ones(P, dtype=torch.long) if i == 2 else None, text=f"text {i}")
        path = DF.write_cache_entry(str(tmp_path), e)
        assert os.path.basename(path) == f"utt{i}.pt" and DF.is_current(path)
        lens[f"utt{i}"] = (int(f["mel_length"]), P)
    assert not DF.is_current(str(tmp_path / "nope.pt"))
    ds = CachedFeatureDataset(str(tmp_path))
    items = [ds[i] for i in range(len(ds))]
    assert [it["audio_file"] for it in items] == ["utt1", "utt2", "utt3"]                   # sorted by length
    for it in items:
        T, P = lens[it["audio_file"]]
        assert it["mel_spec"].shape == (80, T) and it["mel_spec"].dtype == torch.float32 and it["_cache_version"] == 7
        assert it["pitch"].shape == it["energy"].shape == it["stop_token_targets"].shape == (T,)
        assert it["phoneme_indices"].dtype == it["stress_indices"].dtype == it["phoneme_durations"].dtype == torch.long
        assert it["mel_length"] == T and it["phoneme_length"] == P and int(it["phoneme_durations"].sum()) == T
        assert it["text"].startswith("text ") and float(it["stop_token_targets"][-1]) == 1.0
    batch = collate_fn(items)
    assert batch["mel_specs"].shape == (3, 301, 80) and batch["pitches"].shape == batch["energies"].shape == (3, 301)
    assert batch["phoneme_indices"].shape == (3, 30) and batch["mel_lengths"].tolist() == [12, 129, 301]
    assert torch.equal(batch["mel_specs"][1, :129], items[1]["mel_spec"].T) and batch["stress_indices"][1, :9].tolist() == [1] * 9


def test_extractor_argument_checks():
    from kokoro_ruslan_amd.features import check_wave
    check_wave(0, torch.zeros(10))
    for i, bad in enumerate((torch.zeros(2, 10), torch.zeros(10, dtype=torch.int16), torch.zeros(0), [0.0, 1.0])):
        with pytest.raises(ValueError, match=f"waveform {i}"):
            check_wave(i, bad)


@pytest.mark.parametrize("flag, value", [("--n-mels", "64"), ("--hop-length", "512"), ("--sample-rate", "16000"), ("--batch-size", "0"),
                                         ("--max-seq-length", "0")])
def test_precompute_rejects_flags(flag, value, tmp_path, capsys):
    from kokoro.cli import precompute
    with pytest.raises(SystemExit) as e:
        precompute.main(["--wavs", str(tmp_path), "--ids", str(tmp_path / "x.jsonl"), "--cache-dir", str(tmp_path / "c"), flag, value])
    assert e.value.code == 2 and flag in capsys.readouterr().err


def test_precompute_accepts_the_reference_defaults():
    from kokoro.cli import precompute
    p = precompute.build_parser()
    args = p.parse_args(["--wavs", "w", "--ids", "i", "--cache-dir", "c", "--n-mels", "80", "--hop-length", "256", "--sample-rate", "22050",
                         "--force", "--no-variance"])
    precompute.check_args(p, args)
    assert args.force and args.no_variance and args.batch_size == 32 and args.max_seq_length == 1800
