"""FeatureExtractor end to end against features_torch in fp64 on the same fp32 input: pitch and energy after every decision, bit-exact
batch invariance, the all-zero utterance, variance=False, max_seq_length clipping, the hand-over from GriffinLimVocoder, and
kokoro-precompute -> CachedFeatureDataset -> collate_fn -> one train step.

Bounds.  Energy: |delta| <= 1e-5 on every frame (fp32 torch <= 1.8e-6; a variance-adaptor bucket is 1/256 wide).  Pitch: a frame is in
bound when |delta| <= 1e-4 (0.075 Hz, 1/39 of a bucket) and its voiced/unvoiced decision agrees; the tracker takes hard decisions a
last-bit difference can flip and the gap fill and median filter spread, so at most 1 % of the frames of the whole batch may be out of
bound (the reference's own fp32 run against fp64 has none on this signal family).  Linear mel and log-mel of the vocoder hand-over: the
rules of test_features_kernels_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import features_torch as FT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "features.npz")
KEYS = ("mel_spec", "pitch", "energy")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _waves():
    g = np.load(GOLDEN)
    return [torch.from_numpy(g[f"signal_{i}"]).float() / 32768.0 for i in range(len(g["lengths"]))] + [torch.zeros(5000)]


def _extractor():
    from kokoro_ruslan_amd.features import FeatureExtractor
    return FeatureExtractor()


def _check_pitch_energy(got, want):
    total = bad = 0
    for b, (g, w) in enumerate(zip(got, want)):
        T = w["mel_length"]
        assert g["mel_length"] == T and g["mel_spec"].shape == (80, T) and g["pitch"].shape == g["energy"].shape == (T,)
        assert all(g[k].dtype == torch.float32 for k in KEYS)
        de = float((g["energy"].double().cpu() - w["energy"]).abs().max())
        gp, wp = g["pitch"].double().cpu(), w["pitch"]
        out = ((gp - wp).abs() > 1e-4) | ((gp > 0) != (wp > 0))
        print(f"utterance {b}: {T} frames, energy max |delta| {de:.2e}, pitch frames out of bound {int(out.sum())}")
        assert de <= 1e-5, (b, de)
        total += T
        bad += int(out.sum())
    print(f"pitch: {bad} of {total} frames out of bound")
    assert bad <= 0.01 * total, (bad, total)


def test_pitch_and_energy_against_fp64():
    _need_gpu()
    waves = _waves()
    got = _extractor().extract([w.cuda() for w in waves])
    assert sum(g["mel_length"] for g in got) >= 1000
    _check_pitch_energy(got, [FT.extract(w, dtype=torch.float64) for w in waves])


def test_max_seq_length_clipping():
    """Mel and energy statistics over the 64 kept frames, pitch statistics over all frames of the utterance."""
    _need_gpu()
    waves = _waves()
    got = _extractor().extract([w.cuda() for w in waves], max_seq_length=64)
    want = [FT.extract(w, max_seq_length=64, dtype=torch.float64) for w in waves]
    assert [g["mel_length"] for g in got] == [5, 12, 64, 64, 64, 20]
    _check_pitch_energy(got, want)
    full = _extractor().extract([waves[4].cuda()])[0]
    assert torch.equal(got[4]["mel_spec"], full["mel_spec"][:, :64]) and torch.equal(got[4]["pitch"], full["pitch"][:64])
    assert not torch.equal(got[4]["energy"], full["energy"][:64])


def test_batch_invariance_bit_for_bit():
    _need_gpu()
    ext = _extractor()
    waves = [w.cuda() for w in _waves()]
    together = ext.extract(waves)
    rev = ext.extract(waves[::-1])[::-1]
    grouped = ext.extract(waves, max_samples=40000)
    for b, w in enumerate(waves):
        alone = ext.extract([w])[0]
        for k in KEYS:
            assert torch.equal(together[b][k], alone[k]), (b, k)
            assert torch.equal(rev[b][k], alone[k]), (b, k)
            assert torch.equal(grouped[b][k], alone[k]), (b, k)
    assert float(together[3]["pitch"].max()) > 0.0 and float(together[3]["energy"].std()) > 1e-3


def test_all_zero_utterance_is_exact():
    _need_gpu()
    z = _extractor().extract([torch.zeros(5000).cuda(), _waves()[2].cuda()])[0]
    assert z["mel_length"] == 20
    assert torch.equal(z["mel_spec"].cpu(), torch.full((80, 20), 1e-9, dtype=torch.float32).log())
    assert torch.equal(z["pitch"], torch.zeros_like(z["pitch"])) and torch.equal(z["energy"], torch.zeros_like(z["energy"]))


def test_variance_off():
    _need_gpu()
    ext = _extractor()
    waves = [w.cuda() for w in _waves()[:3]]
    off, on = ext.extract(waves, variance=False), ext.extract(waves)
    for a, b in zip(off, on):
        assert torch.equal(a["mel_spec"], b["mel_spec"])
        assert torch.equal(a["pitch"], torch.zeros_like(b["pitch"])) and torch.equal(a["energy"], torch.zeros_like(b["energy"]))


def test_argument_checks():
    _need_gpu()
    ext = _extractor()
    w = torch.zeros(3000)
    with pytest.raises(ValueError, match="waveform 1"):
        ext.extract([w, torch.zeros(2, 3000)])
    with pytest.raises(ValueError, match="waveform 2"):
        ext.extract([w, w, torch.zeros(3000, dtype=torch.int16)])
    with pytest.raises(ValueError, match="waveform 0"):
        ext.extract([torch.zeros(0)])
    with pytest.raises(ValueError, match="max_seq_length"):
        ext.extract([w], max_seq_length=0)


def test_hand_over_from_griffin_lim():
    """extract() on real vocoder output: a T-frame mel vocoded to 256 (T - 1) samples comes back as exactly T frames and meets the
    linear-mel and log-mel rules against fp64 on that waveform."""
    _need_gpu()
    from kokoro_ruslan_amd import griffinlim_torch as GT
    from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
    T = 120
    mel = GT.harmonic_logmel(T, seed=3, f0=140.0).float().cuda()
    wave = GriffinLimVocoder().vocode([mel], n_iter=8, generator=torch.Generator().manual_seed(1))[0]
    assert wave.shape == (256 * (T - 1),)
    g = _extractor().extract([wave], keep_linear=True)[0]
    assert g["mel_length"] == T == 1 + 256 * (T - 1) // 256
    w = FT.extract(wave.cpu(), dtype=torch.float64)
    rel = float((g["mel_linear"].double().cpu() - w["mel_linear"]).norm() / w["mel_linear"].norm())
    edge = [0, 1, -2, -1]
    rel_e = float((g["mel_linear"].double().cpu()[:, edge] - w["mel_linear"][:, edge]).norm() / w["mel_linear"][:, edge].norm())
    allowed = float((FT.extract(wave.cpu(), dtype=torch.float32)["mel_spec"].double() - w["mel_spec"]).abs().max())
    err = float((g["mel_spec"].double().cpu() - w["mel_spec"]).abs().max())
    print(f"hand-over: linear mel relative L2 {rel:.2e} (edges {rel_e:.2e}), log-mel max error {err:.2e}, fp32 torch {allowed:.2e}")
    assert rel <= 1e-5 and rel_e <= 1e-5 and err <= 4.0 * allowed


def test_kokoro_precompute_feeds_a_train_step(tmp_path):
    """kokoro-precompute in a fresh child process, then CachedFeatureDataset -> collate_fn -> one forward_backward at tiny dims;
    a second run skips everything."""
    _need_gpu()
    from kokoro.data.cached import CachedFeatureDataset, collate_fn
    from kokoro.inference.audio import write_wav
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    g = torch.Generator().manual_seed(4)
    lines = []
    for i, n in enumerate((9000, 5200, 14000)):
        write_wav(str(wavs / f"u{i}.wav"), FT.test_signal(n, seed=20 + i, f0=100.0 + 60 * i), 22050)
        P = 5 + 3 * i
        rec = {"name": f"u{i}", "phoneme_indices": torch.randint(1, 59, (P,), generator=g).tolist(), "text": f"utterance {i}"}
        if i == 1:
            rec["phoneme_durations"] = [2] * P
        lines.append(json.dumps(rec) + "\n")
    ids = tmp_path / "u.jsonl"
    ids.write_text("".join(lines))
    cache = tmp_path / "cache"
    cmd = [sys.executable, "-m", "kokoro.cli.precompute", "--wavs", str(wavs), "--ids", str(ids), "--cache-dir", str(cache)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "3 computed, 0 skipped, 0 failed" in r.stdout, r.stdout
    ds = CachedFeatureDataset(str(cache))
    assert len(ds) == 3
    items = [ds[i] for i in range(3)]
    assert sorted(it["mel_length"] for it in items) == [1 + 5200 // 256, 1 + 9000 // 256, 1 + 14000 // 256]
    for it in items:
        assert int(it["phoneme_durations"].sum()) == it["mel_length"] and it["_cache_version"] == 7
        assert float(it["pitch"].max()) > 0 and float(it["energy"].max()) == 1.0
    batch = collate_fn(items)
    d = ModelDims(vocab=59, mel=80, hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32, var_kernel=3,
                  var_bins=16, max_len=300)
    e = KokoroEngine(d, StepHyper(), math_mode="f32", total_steps=100, seed=5)
    e.zero_grad()
    out = e.forward_backward({k: v.cuda() for k, v in batch.items()})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["losses"]).all()), out["losses"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "0 computed, 3 skipped, 0 failed" in r.stdout, r.stdout + r.stderr
