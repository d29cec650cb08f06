"""Writing the feature cache: what the reference's dataset does around the acoustic front-end when it builds a sample
(data/dataset.py:581-606, :644-672, :737-784, :849-862).  `load_wav` reads a .wav by the reference's dtype rules, `stop_token_targets`
and `fallback_durations` restate build_stop_token_targets and _build_fallback_durations, `cache_entry` assembles a schema-v7 entry from
the device extractor's output and `write_cache_entry` saves it as <audio_file>.pt, the file kokoro.data.cached reads.  `load_wav_any`
reads a .wav at any rate for the callers that resample on the device (kokoro-precompute --resample).  The phonemizer and MFA
alignment are out of scope: phoneme ids (and durations, when aligned) are given.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

from kokoro.data.cached import FEATURE_CACHE_VERSION, reference_reconcile

SAMPLE_RATE = 22050


def load_wav_any(path: str):
    """(sample rate, mono fp32 samples) of a .wav at any rate, un-normalised: int16 / 32768, int32 / 2^31, anything else cast to fp32;
    channels averaged (dataset.py:644-669)."""
    from scipy.io import wavfile
    sr, a = wavfile.read(str(path))
    if a.dtype == np.int16:
        a = a.astype(np.float32) / 32768.0
    elif a.dtype == np.int32:
        a = a.astype(np.float32) / 2147483648.0
    else:
        a = a.astype(np.float32)
    x = torch.from_numpy(a)
    if x.dim() == 2:
        x = x.T.mean(dim=0) if x.shape[1] > 1 else x[:, 0]
    return int(sr), x.contiguous()


def load_wav(path: str) -> torch.Tensor:
    """Mono fp32 samples of a .wav, un-normalised, by load_wav_any's rules.  A sample rate other than 22050 Hz is an error: resampling
    is out of scope here (kokoro-precompute --resample does it on the device)."""
    sr, x = load_wav_any(path)
    if sr != SAMPLE_RATE:
        raise ValueError(f"{path}: sample rate {sr} Hz, expected {SAMPLE_RATE}; resampling is out of scope here, resample the corpus "
                         f"first (the reference does it with torchaudio)")
    return x


def stop_token_targets(T: int, tail: int = 4, decay: float = 0.5) -> torch.Tensor:
    """build_stop_token_targets: 1 at the last frame, decay^k at the k-th frame before it for k <= tail (dataset.py:32-64)."""
    t = torch.zeros(T, dtype=torch.float32)
    if T > 0:
        n = min(tail + 1, T)
        t[T - n:] = (decay ** torch.arange(n, dtype=torch.float32)).flip(0)
    return t


def fallback_durations(num_phonemes: int, num_mel_frames: int) -> torch.Tensor:
    """_build_fallback_durations: frames spread evenly over the phonemes, the remainder one each to the first ones (dataset.py:581-606)."""
    P, T = max(0, int(num_phonemes)), max(0, int(num_mel_frames))
    if P == 0:
        return torch.zeros((0,), dtype=torch.long)
    d = torch.full((P,), T // P, dtype=torch.long)
    d[:T % P] += 1
    return d


def cache_entry(features: Dict, audio_file: str, phoneme_indices: torch.Tensor, stress_indices: Optional[torch.Tensor] = None,
                phoneme_durations: Optional[torch.Tensor] = None, text: str = "") -> Dict:
    """A schema-v7 cache entry (dataset.py:849-862) from one FeatureExtractor.extract() result; tensors on the CPU.  Given durations
    are reconciled with the frame count by the reference's rule (:761-768), absent ones are the fallback estimate."""
    T = int(features["mel_length"])
    ids = torch.as_tensor(phoneme_indices, dtype=torch.long)
    if ids.dim() != 1:
        raise ValueError(f"{audio_file}: phoneme_indices must be 1-D, got shape {tuple(ids.shape)}")
    stress = torch.zeros_like(ids) if stress_indices is None else torch.as_tensor(stress_indices, dtype=torch.long)
    if stress.shape != ids.shape:
        raise ValueError(f"{audio_file}: {stress.shape[0]} stress_indices for {ids.shape[0]} phonemes")
    if phoneme_durations is None:
        dur = fallback_durations(ids.shape[0], T)
    else:
        dur = torch.as_tensor(phoneme_durations, dtype=torch.long)
        if dur.shape != ids.shape:
            raise ValueError(f"{audio_file}: {dur.shape[0]} phoneme_durations for {ids.shape[0]} phonemes")
        dur = reference_reconcile(dur, T)
    cpu = lambda k: features[k].detach().to("cpu", torch.float32).contiguous()
    return {"mel_spec": cpu("mel_spec"), "phoneme_indices": ids, "stress_indices": stress, "phoneme_durations": dur,
            "stop_token_targets": stop_token_targets(T), "pitch": cpu("pitch"), "energy": cpu("energy"), "text": text,
            "audio_file": audio_file, "mel_length": T, "phoneme_length": int(ids.shape[0]), "_cache_version": FEATURE_CACHE_VERSION}


def cache_path(cache_dir: str, audio_file: str) -> str:
    return os.path.join(str(cache_dir), f"{audio_file}.pt")


def is_current(path: str) -> bool:
    """True when `path` holds an entry of the current cache version (what a run without --force skips)."""
    if not os.path.exists(path):
        return False
    try:
        return torch.load(path, map_location="cpu", weights_only=False).get("_cache_version") == FEATURE_CACHE_VERSION
    except Exception:
        return False


def write_cache_entry(cache_dir: str, entry: Dict) -> str:
    os.makedirs(str(cache_dir), exist_ok=True)
    path = cache_path(cache_dir, entry["audio_file"])
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(entry, tmp)
    os.replace(tmp, path)
    return path
