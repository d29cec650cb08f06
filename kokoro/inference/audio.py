"""Mels to audio: the engine-side counterpart of the reference's vocoder step (inference/inference.py:588-634, 684-739) and of
AudioUtils.save_audio.  `vocode` runs a batch of mels through a kokoro_ruslan_amd.vocoder.HifiganVocoder or a
kokoro_ruslan_amd.griffinlim.GriffinLimVocoder; `denoise` takes the vocoder's stationary noise floor out of a batch of waveforms with a
kokoro_ruslan_amd.denoise.SpectralDenoiser; `normalise_loudness` brings a batch of waveforms to one integrated loudness under a peak
ceiling with a kokoro_ruslan_amd.loudness.LoudnessNormaliser; `finish_mels` and `join_chunks` are the two ends of long-form synthesis
(:569-648): the health check, clamp and trailing-silence trim of every chunk's mel with a kokoro_ruslan_amd.longform.MelFinisher, and
the chunk waveforms of every document joined with silence between them; `write_wav` writes one waveform as 16-bit PCM."""
from __future__ import annotations

import math
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


def finish_mels(finisher, mels: Sequence[torch.Tensor]):
    """(mels clamped to [-11.5, 2] with their trailing silence trimmed (inference.py:588-619), left on the device, info): in input
    order; info[b] = {"frames", "kept", "last_voiced", "threshold", "min", "max", "mean", "std", "nan", "flat"}, the statistics those
    of the mel as it came (:569-580)."""
    return finisher.finish(list(mels))


def join_chunks(waves: Sequence[torch.Tensor], documents: Sequence[Sequence[int]], sample_rate: int, gap_ms: float = 150.0,
                fade_ms: float = 0.0):
    """(one waveform per document, peaks): documents[d] lists the indices into `waves` of a document's chunks in playback order;
    int(sample_rate gap_ms / 1000) zero samples go between consecutive chunks (the reference's 0.15 s, :645) and none at a
    document's ends.  fade_ms > 0 fades every chunk in and out over that time (at most half the chunk); 0 is the reference's plain
    concatenation.  peaks: fp32 [len(waves)], max |x| of every chunk (:637).  Everything stays on the device."""
    for name, v in (("gap_ms", gap_ms), ("fade_ms", fade_ms)):
        if not math.isfinite(float(v)) or v < 0:
            raise ValueError(f"{name} must be finite and >= 0, not {v!r}")
    from kokoro_ruslan_amd.longform import join
    waves = list(waves)
    device = waves[0].device if waves and isinstance(waves[0], torch.Tensor) and waves[0].is_cuda else "cuda"
    return join(waves, documents, int(sample_rate * gap_ms / 1000), int(sample_rate * fade_ms / 1000), device=device)


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
