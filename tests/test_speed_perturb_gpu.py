"""Train-time speed perturbation through the loader and the trainer: a temporary corpus of short synthetic wavs with its feature cache
(written through kokoro.data.features), BatchPrefetcher with a SpeedPerturbation, and one train_epoch at tiny model dimensions."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N_UTT = 12


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """{root}/wavs/u00.wav ... (tones plus noise, 0.3-1.5 s, int16 at 22050 Hz) and {root}/.feature_cache/ from the device extractor;
    even utterances carry aligned durations, odd ones the fallback estimate."""
    _need_gpu()
    from scipy.io import wavfile
    from kokoro.data import features as DF
    from kokoro_ruslan_amd.features import FeatureExtractor
    root = tmp_path_factory.mktemp("corpus")
    (root / "wavs").mkdir()
    g = torch.Generator().manual_seed(7)
    waves = []
    for i in range(N_UTT):
        n = int(22050 * (0.3 + 1.2 * i / (N_UTT - 1)))
        t = torch.arange(n, dtype=torch.float64) / 22050
        x = 0.4 * torch.sin(2 * math.pi * (110.0 + 15 * i) * t) + 0.2 * torch.sin(2 * math.pi * (900.0 + 70 * i) * t)
        x = x + 0.03 * torch.randn(n, generator=g, dtype=torch.float64)
        a = (x * 30000).round().clamp(-32768, 32767).to(torch.int16).numpy()
        wavfile.write(root / "wavs" / f"u{i:02d}.wav", 22050, a)
        waves.append(DF.load_wav(root / "wavs" / f"u{i:02d}.wav"))
    feats = FeatureExtractor().extract(waves)
    for i, ft in enumerate(feats):
        P = 4 + i % 5
        ids = torch.randint(1, 59, (P,), generator=g)
        dur = None
        if i % 2 == 0:
            dur = DF.fallback_durations(P, ft["mel_length"])
            dur[0] += 2
            dur[-1] -= 2
        DF.write_cache_entry(root / ".feature_cache", DF.cache_entry(ft, f"u{i:02d}", ids, None, dur, f"utterance {i}"))
    return root


def _dataset(corpus):
    from kokoro.data.cached import CachedFeatureDataset
    return CachedFeatureDataset(str(corpus / ".feature_cache"))


def _drain(ds, batches, perturb, epoch=0):
    from kokoro.training.trainer import BatchPrefetcher
    out = []
    pf = BatchPrefetcher(ds, batches, torch.device("cuda", torch.cuda.current_device()), perturb=perturb, epoch=epoch)
    for views, expanded in pf:
        torch.cuda.current_stream().synchronize()
        out.append(({k: v.clone() for k, v in views.items()}, expanded))
    return out, pf


def test_every_row_perturbed(corpus):
    _need_gpu()
    from kokoro.data.augment import SpeedPerturbation, mel_frames, perturbed_samples
    from kokoro.data.features import fallback_durations, load_wav, stop_token_targets
    from kokoro_ruslan_amd.features import FeatureExtractor
    ds = _dataset(corpus)
    sp = SpeedPerturbation(ds, str(corpus / "wavs"), prob=1.0, spread=0.1, seed=0)
    batches = [[0, 5, 11, 2], [7, 1, 9, 4], [3, 10, 6, 8]]
    got, pf = _drain(ds, batches, sp, epoch=2)
    assert pf.perturbed_rows == N_UTT and len(got) == 3
    ext = FeatureExtractor()
    for idxs, (b, expanded) in zip(batches, got):
        Tmax = 0
        for r, i in enumerate(idxs):
            f = sp.factor(i, 2)
            assert f != 1.0 and 0.9 <= f <= 1.1
            wav = load_wav(sp.wav_path(i))
            T = mel_frames(perturbed_samples(wav.shape[0], f), 1800)
            Tmax = max(Tmax, T)
            P = int(ds[i]["phoneme_length"])
            assert int(b["mel_lengths"][r]) == T == sp.perturbed_length(i, 2)
            assert int(b["phoneme_lengths"][r]) == P and torch.equal(b["phoneme_indices"][r, :P].cpu(), ds[i]["phoneme_indices"])
            dur = b["phoneme_durations"][r, :P].cpu()
            cached = ds[i]["phoneme_durations"]
            if torch.equal(cached, fallback_durations(P, ds[i]["mel_length"])):
                assert torch.equal(dur, fallback_durations(P, T))
            else:
                scaled = torch.clamp((cached.float() / f).round().long(), min=1)
                assert torch.equal(dur[:-1], scaled[:-1])
            assert int(dur.min()) >= 1
            assert int(dur.sum()) == T or (int(dur.sum()) > T and int(dur[-1]) == 1)     # larger only where the clamp held the last one at 1
            assert torch.equal(b["stop_token_targets"][r, :T].cpu(), stop_token_targets(T)) and float(b["stop_token_targets"][r, T - 1]) == 1.0
            want = ext.extract_perturbed([wav.cuda()], [f])[0]
            assert want["mel_length"] == T
            assert torch.equal(b["mel_specs"][r, :T], want["mel_spec"].T), (i, "mel")
            assert torch.equal(b["pitches"][r, :T], want["pitch"]) and torch.equal(b["energies"][r, :T], want["energy"]), i
            assert not bool(b["mel_specs"][r, T:].any()) and not bool(b["pitches"][r, T:].any()) and not bool(b["stop_token_targets"][r, T:].any())
        assert b["mel_specs"].shape == (4, Tmax, 80)
        assert expanded == int(b["phoneme_durations"].sum(1).max())


def test_unperturbed_paths_equal_the_cache_loader(corpus):
    """prob = 0 and no perturbation at all give the same batches, bit for bit; with prob = 0.5 the unperturbed rows still do."""
    _need_gpu()
    from kokoro.data.augment import SpeedPerturbation
    from kokoro.data.cached import collate_fn
    ds = _dataset(corpus)
    batches = [[0, 5, 11, 2], [7, 1, 9, 4], [3, 10, 6, 8]]
    plain, _ = _drain(ds, batches, None)
    off, pf = _drain(ds, batches, SpeedPerturbation(ds, str(corpus / "wavs"), prob=0.0))
    assert pf.perturbed_rows == 0
    for idxs, (a, ea), (b, eb) in zip(batches, plain, off):
        want = collate_fn([ds[i] for i in idxs])
        assert ea == eb and set(a) == set(b) == set(want)
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k].cpu(), want[k]), k
    sp = SpeedPerturbation(ds, str(corpus / "wavs"), prob=0.5)
    half, pf = _drain(ds, batches, sp, epoch=1)
    hit = [i for i in range(N_UTT) if sp.factor(i, 1) != 1.0]
    assert 0 < len(hit) < N_UTT and pf.perturbed_rows == len(hit)
    for idxs, (b, _) in zip(batches, half):
        for r, i in enumerate(idxs):
            if i not in hit:
                T = int(ds[i]["mel_length"])
                assert int(b["mel_lengths"][r]) == T and torch.equal(b["mel_specs"][r, :T].cpu(), ds[i]["mel_spec"].T)
                assert torch.equal(b["pitches"][r, :T].cpu(), ds[i]["pitch"])


def _config(corpus, out, **kw):
    from kokoro.training.config import TrainingConfig
    return TrainingConfig(data_dir=str(corpus), output_dir=str(out), n_mels=80, hidden_dim=128, n_encoder_layers=1, n_decoder_layers=1,
                          n_heads=2, encoder_ff_dim=96, decoder_ff_dim=96, max_decoder_seq_len=400, variance_filter_size=32,
                          n_variance_bins=16, batch_size=4, use_dynamic_batching=False, num_epochs=1, validation_split=0.0,
                          gradient_accumulation_steps=1, use_mixed_precision=False, **kw)


def test_train_epoch_with_perturbation(corpus, tmp_path):
    _need_gpu()
    from kokoro.training.trainer import KokoroTrainer
    tr = KokoroTrainer(_config(corpus, tmp_path / "m", use_speed_perturbation=True, speed_perturb_prob=0.5))
    assert tr.perturb is not None and tr.perturb.prob == 0.5
    loss = tr.train_epoch(0)
    assert math.isfinite(loss)
    assert 0 < tr.last_prefetch.perturbed_rows < N_UTT
    assert tr.engine.opt_stats()["skipped"] == 0 and tr.engine.opt_stats()["attempt"] == 3.0


def test_perturbation_needs_the_flag_and_the_audio(corpus, tmp_path):
    """Off when the config says so, and off (one log line, the cache-only loop) when {data_dir}/wavs/ does not exist."""
    _need_gpu()
    import shutil
    from kokoro.training.trainer import KokoroTrainer
    assert KokoroTrainer(_config(corpus, tmp_path / "a", use_speed_perturbation=False)).perturb is None
    bare = tmp_path / "bare"
    shutil.copytree(corpus / ".feature_cache", bare / ".feature_cache")
    tr = KokoroTrainer(_config(bare, tmp_path / "b", use_speed_perturbation=True))
    assert tr.perturb is None
    assert math.isfinite(tr.train_epoch(0)) and tr.last_prefetch.perturbed_rows == 0
