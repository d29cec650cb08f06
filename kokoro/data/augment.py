"""Train-time speed perturbation, the host side: what the reference's dataset decides and rebuilds around the resampled audio when it
perturbs a training sample (data/dataset.py:613-627 the draw, :755-768 the durations, :777-784 the stop targets).  The audio itself
(normalise, resample 22050 -> int(22050 f), normalise, features) runs on the device: FeatureExtractor.extract_perturbed.

The reference draws from the process-global `random` module as samples are fetched, so its factors depend on the fetch order.  Here
the draws of utterance i in epoch e come from `random.Random` seeded by (seed, e, i), in the reference's order (`random() < prob`,
then `1 + uniform(-range, range)`): a pure function, so every rank of a data-parallel run can compute any utterance's factor and its
perturbed length without communication.
"""
from __future__ import annotations

import os
import random
from typing import Dict, Optional

import numpy as np
import torch

from kokoro.data.cached import reference_reconcile
from kokoro.data.features import SAMPLE_RATE, fallback_durations, load_wav, stop_token_targets

N_FFT, HOP = 1024, 256


def draw_factor(seed: int, epoch: int, index: int, prob: float, spread: float) -> float:
    """The speed factor of dataset index `index` in `epoch`: 1.0 (not perturbed) unless random() < prob, then 1 + uniform(-spread,
    spread) (dataset.py:616-627)."""
    rng = random.Random(f"kokoro-speed-perturb:{int(seed)}:{int(epoch)}:{int(index)}")
    if rng.random() < prob:
        return 1.0 + rng.uniform(-spread, spread)
    return 1.0


def perturbed_samples(num_samples: int, factor: float, sample_rate: int = SAMPLE_RATE) -> int:
    """Samples after resampling sample_rate -> int(sample_rate factor): ceil(n L / o) over the reduced rates."""
    new = int(sample_rate * factor)
    return (new * int(num_samples) + sample_rate - 1) // sample_rate        # (ceil(new L / orig) = ceil(n L / o): the gcd cancels)


def mel_frames(num_samples: int, max_seq_length: int) -> int:
    """Frames the feature extractor keeps: the waveform zero-padded to the window, centre = True, cut to max_seq_length."""
    return min(1 + max(int(num_samples), N_FFT) // HOP, int(max_seq_length))


def rescale_durations(durations: torch.Tensor, factor: float, frames: int, cached_frames: int) -> torch.Tensor:
    """Durations of a perturbed sample with `frames` mel frames (dataset.py:752-775).  The reference rescales an MFA alignment,
    clamp(round(d / f), min = 1), and reconciles it with the frame count; without an alignment it spreads the new frame count evenly.
    The cache does not say which it was, so durations that equal the even spread of the cached frame count are taken as unaligned."""
    d = torch.as_tensor(durations, dtype=torch.long)
    if torch.equal(d, fallback_durations(d.shape[0], cached_frames)):
        return fallback_durations(d.shape[0], frames)
    scaled = d.float() / factor
    return reference_reconcile(torch.clamp(scaled.round().long(), min=1), frames)


class SpeedPerturbation:
    """Per-epoch speed perturbation of a CachedFeatureDataset whose audio lies in `wav_dir` as <audio_file>.wav."""

    def __init__(self, dataset, wav_dir: str, prob: float = 0.5, spread: float = 0.1, seed: int = 0, max_seq_length: int = 1800,
                 memory_cache: bool = True):
        self.dataset, self.wav_dir, self.prob, self.spread, self.seed = dataset, str(wav_dir), float(prob), float(spread), int(seed)
        self.max_seq_length = int(max_seq_length)
        self._len: Dict[int, int] = {}
        self._mem: Optional[Dict[int, np.ndarray]] = {} if memory_cache else None
        self._extractor = None
        missing = [i for i in range(len(dataset)) if not os.path.exists(self.wav_path(i))]
        if missing:
            raise FileNotFoundError(f"speed perturbation: {len(missing)} of {len(dataset)} training utterances have no audio under "
                                    f"{self.wav_dir} (first: {os.path.basename(self.wav_path(missing[0]))}); set "
                                    f"use_speed_perturbation = False to train from the cache alone")

    def wav_path(self, i: int) -> str:
        return os.path.join(self.wav_dir, f"{self.dataset.samples[i]['file'].stem}.wav")       # the cache file is <audio_file>.pt

    def factor(self, i: int, epoch: int) -> float:
        return draw_factor(self.seed, epoch, i, self.prob, self.spread)

    def wav_length(self, i: int) -> int:
        n = self._len.get(i)
        if n is None:
            from scipy.io import wavfile
            _, a = wavfile.read(self.wav_path(i), mmap=True)              # (the header and a mapping: the samples are not read)
            n = self._len[i] = int(a.shape[0])
        return n

    def perturbed_length(self, i: int, epoch: int) -> int:
        """Mel frames of utterance i in `epoch`: the cached count, or what the perturbed audio gives."""
        f = self.factor(i, epoch)
        if f == 1.0:
            return int(self.dataset.samples[i]["audio_length"])
        return mel_frames(perturbed_samples(self.wav_length(i), f), self.max_seq_length)

    def samples(self, i: int) -> np.ndarray:
        """The utterance's mono samples by load_wav's rules: int16 (x = a / 32768) when that is exact, which halves what
        use_memory_cache keeps, else fp32."""
        if self._mem is not None and i in self._mem:
            return self._mem[i]
        x = load_wav(self.wav_path(i)).numpy()
        q = np.rint(x * np.float32(32768.0))
        a = q.astype(np.int16) if (np.abs(q) <= 32767).all() and np.array_equal(q.astype(np.float32) / np.float32(32768.0), x) else x
        self._len[i] = int(a.shape[0])
        if self._mem is not None:
            self._mem[i] = a
        return a

    def extractor(self, device):
        if self._extractor is None:
            from kokoro_ruslan_amd.features import FeatureExtractor
            self._extractor = FeatureExtractor(device)
        return self._extractor

    def item(self, i: int, epoch: int, cached: Dict) -> Optional[Dict]:
        """None when utterance i is not perturbed in `epoch`; else the sample's host-side fields for the collate (ids and stress as
        cached, rescaled durations, stop targets and mel_length for the perturbed frame count; mel, pitch and energy are zero
        placeholders the loader overwrites on the device) plus "_perturb" = (samples, factor)."""
        f = self.factor(i, epoch)
        if f == 1.0:
            return None
        a = self.samples(i)
        T = mel_frames(perturbed_samples(a.shape[0], f), self.max_seq_length)
        M = int(cached["mel_spec"].shape[0])
        dur = rescale_durations(cached["phoneme_durations"], f, T, int(cached["mel_length"]))
        stop = stop_token_targets(T)
        zeros = lambda *shape: np.broadcast_to(np.float32(0.0), shape)
        return {"mel_spec": cached["mel_spec"], "phoneme_indices": cached["phoneme_indices"], "stress_indices": cached["stress_indices"],
                "phoneme_durations": dur, "stop_token_targets": stop, "mel_length": T, "phoneme_length": cached["phoneme_length"],
                "audio_file": cached.get("audio_file"), "_perturb": (a, f),
                "_np": {"mel": zeros(T, M), "pitch": zeros(T), "energy": zeros(T), "stop": stop.numpy(),
                        "ids": cached["phoneme_indices"].numpy(), "dur": dur.numpy(), "stress": cached["stress_indices"].numpy()}}
