#!/usr/bin/env python3
"""Record the reference's pitch, energy, stop targets and fallback durations on the seeded test signals: tests/golden/features.npz.

Runs only where the reference's sources are available (on the CPU):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_features_golden.py <reference>/src

It imports the reference's PitchExtractor, EnergyExtractor, build_stop_token_targets and RuslanDataset._build_fallback_durations
(torchaudio stubbed as in make_golden.py: none of the four touches it), runs them in fp32 on kokoro_ruslan_amd.features_torch's
test signals and writes inputs and recorded results only.  The energy is the reference's on the fp64 linear mel of features_torch cast
to fp32: torchaudio's MelSpectrogram itself is not executed, the mel is pinned to its definition (melscale_fbanks and torch.stft).
"""
import os
import sys
import types
from unittest import mock

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ["KOKORO_REFERENCE_SRC"])

import numpy as np
import torch

tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
sys.modules["torch.utils.tensorboard"] = tb
for name in ("torchaudio", "torchaudio.transforms", "torchaudio.functional"):
    sys.modules[name] = mock.MagicMock()

from kokoro.model.variance_predictor import EnergyExtractor, PitchExtractor        # noqa: E402
from kokoro.data.dataset import RuslanDataset, build_stop_token_targets            # noqa: E402
from kokoro_ruslan_amd import features_torch as FT                                 # noqa: E402

# samples, seed, f0: shorter than both windows; short; 1.5 s; 3.5 s; 6.5 s (1006 mel frames together)
SIGNALS = [(700, 1, 70.0), (3000, 2, 500.0), (33000, 3, 110.0), (77000, 4, 180.0), (143000, 5, 290.0)]
CLIP = 64
STOP_T = [0, 1, 3, 5, 6, 64, 301]
FALLBACK = [(0, 10), (7, 0), (7, 5), (7, 7), (7, 23), (40, 559), (1, 12)]

out = {"lengths": np.array([s[0] for s in SIGNALS], dtype=np.int64), "clip": np.int64(CLIP)}
for i, (n, seed, f0) in enumerate(SIGNALS):
    x16 = torch.round(FT.test_signal(n, seed, f0) * 32767.0).clamp(-32768, 32767).to(torch.int16)
    wave = x16.float() / 32768.0
    audio = FT.normalise(wave, torch.float32)                                       # dataset.py:672, :688-690
    T = FT.mel_frames(n)
    p = PitchExtractor.extract_pitch(audio, sample_rate=22050, hop_length=256, fmin=50.0, fmax=800.0)
    assert p.dtype == torch.float32 and p.shape[0] == FT.pitch_frames(n) and float(p.max()) > 0.0
    p = torch.cat([p[:T], torch.zeros(max(T - p.shape[0], 0))])                     # dataset.py:802-806
    lin = FT.mel_linear(FT.normalise(wave, torch.float64)).float()
    assert lin.shape == (80, T)
    e = EnergyExtractor.extract_energy_from_mel(lin.T, log_domain=False)
    e_clip = EnergyExtractor.extract_energy_from_mel(lin[:, :CLIP].T, log_domain=False)
    out[f"signal_{i}"] = x16.numpy()
    out[f"pitch_{i}"] = p.numpy()
    out[f"energy_{i}"] = e.numpy()
    out[f"energy_clip_{i}"] = e_clip.numpy()
    print(f"signal {i}: {n} samples, {T} frames, voiced {int((p > 0).sum())}")
for T in STOP_T:
    out[f"stop_{T}"] = build_stop_token_targets(T, tail=4, decay=0.5).numpy()
out["fallback_cases"] = np.array(FALLBACK, dtype=np.int64)
for P, T in FALLBACK:
    out[f"fallback_{P}_{T}"] = RuslanDataset._build_fallback_durations(P, T).numpy()
path = os.path.join(HERE, "features.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
