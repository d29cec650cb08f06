"""Mels to audio: the engine-side counterpart of the reference's vocoder step (inference/inference.py:588-634, 684-739) and of
AudioUtils.save_audio.  `vocode` runs a batch of mels through a kokoro_ruslan_amd.vocoder.HifiganVocoder or a
kokoro_ruslan_amd.griffinlim.GriffinLimVocoder; `denoise` takes the vocoder's stationary noise floor out of a batch of waveforms with a
kokoro_ruslan_amd.denoise.SpectralDenoiser; `normalise_loudness` brings a batch of waveforms to one integrated loudness under a peak
ceiling with a kokoro_ruslan_amd.loudness.LoudnessNormaliser; `write_wav` writes one waveform as 16-bit PCM."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch


def vocode(vocoder, mels: Sequence[torch.Tensor], clamp: bool = True, **kwargs) -> List[torch.Tensor]:
    """Waveforms of mels [frames_b, n_mels], in input order.  clamp: the reference's unconditional clamp(-11.5, 2.0) before the
    vocoder (inference.py:590).  kwargs go to vocoder.vocode (HiFi-GAN: max_samples; Griffin-Lim: n_iter, generator, ...)."""
    if clamp:
        mels = [torch.clamp(m, min=-11.5, max=2.0) for m in mels]
    return vocoder.vocode(list(mels), **kwargs)


def denoise(denoiser, waves: Sequence[torch.Tensor], strength: float = 0.005) -> List[torch.Tensor]:
    """The waveforms less `strength` times the denoiser's bias spectrum in every STFT frame (phase kept), in input order and of the same
    lengths.  The denoiser's bias must be set (SpectralDenoiser.bias_from_vocoder, once per vocoder)."""
    return denoiser.denoise(list(waves), strength=strength)


def normalise_loudness(normaliser, waves: Sequence[torch.Tensor], target_lufs: float = -23.0, peak_db: float = -1.0):
    """(waveforms scaled to `target_lufs` integrated loudness (ITU-R BS.1770-4) with the peak held at or under `peak_db` dB of full
    scale, info): in input order and of the same lengths; info[b] = {"start", "end", "measured", "gain", "limited"}.  A waveform too
    short or too quiet to measure is returned as it is.  Write the result with write_wav(..., normalise=False): the peak
    normalisation would undo the level."""
    return normaliser.normalise(list(waves), target_lufs=target_lufs, peak_db=peak_db)


def write_wav(path: str, audio, sample_rate: int, normalise: bool = True) -> None:
    """AudioUtils.save_audio's scipy path: peak-normalise (not below a peak of 1e-8), scale by 32767, write int16 PCM mono.
    normalise=False keeps the level (audio whose loudness has been set): clip to [-1, 1], scale by 32767, round to nearest."""
    from scipy.io import wavfile
    a = audio.detach().float().cpu().reshape(-1) if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio)).float().reshape(-1)
    if not normalise:
        wavfile.write(str(path), int(sample_rate), np.rint(a.clamp(-1.0, 1.0).numpy() * 32767).astype(np.int16))
        return
    peak = torch.max(torch.abs(a)) if a.numel() else torch.tensor(0.0)
    if float(peak) >= 1e-8:
        a = a / peak
    wavfile.write(str(path), int(sample_rate), (a.numpy() * 32767).astype(np.int16))
