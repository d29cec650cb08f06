"""Spectral denoising of vocoded audio on the device, on the kernels of csrc/kk_denoise.hip.

A HiFi-GAN generator that was not trained on this acoustic model's mels leaves a stationary, tonal noise floor in its output.
`SpectralDenoiser` is the bias denoiser of the HiFi-GAN / WaveGlow ecosystem: vocode a silent mel once, take the magnitude spectrum of
what comes out as the vocoder's bias, and subtract a small multiple of it from the magnitude of every synthesized waveform, keeping
the phase (the method and its constants: denoise_torch.py, the fp64 restatement).  The waveforms of one call are packed back to back
and run through one launch; every sum runs in an order fixed by the sample's position in its own utterance, so a waveform's bits do
not depend on the rest of the batch.  All arithmetic is fp32.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.stft import HOP, N_BINS, N_FFT, N_MELS, device_tables

MIN_SAMPLES = N_FFT                     # the reflect padding and the five frames of the shortest bias: a 4-frame HiFi-GAN mel
DEFAULT_STRENGTH = 0.005


def check_strength(strength: float) -> float:
    s = float(strength)
    if not math.isfinite(s) or s < 0:
        raise ValueError(f"strength must be finite and >= 0, not {strength!r}")
    return s


class SpectralDenoiser:
    """set_bias / bias_from_vocoder, then denoise(list of waveforms [samples_b >= 1024]) -> denoised waveforms of the same lengths."""

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        self.window, self.tw = device_tables(self.device)
        self.tile_frames = int(kk.load().kk_denoise_tile_frames())
        self.bias: Optional[torch.Tensor] = None

    def set_bias(self, b: torch.Tensor) -> torch.Tensor:
        """The bias spectrum [513]: finite and >= 0.  Kept as fp32 on the device."""
        b = torch.as_tensor(b)
        if tuple(b.shape) != (N_BINS,):
            raise ValueError(f"bias of shape {tuple(b.shape)}, expected [{N_BINS}]")
        if not bool(torch.isfinite(b).all()) or bool((b < 0).any()):
            raise ValueError("bias must be finite and >= 0 in every bin")
        self.bias = b.detach().to(self.device, torch.float32).contiguous()
        return self.bias

    def bias_from_vocoder(self, vocoder, level: float = -11.5, frames: int = 88) -> torch.Tensor:
        """The bias of `vocoder`: |stft| of what it makes of a constant mel of `frames` frames at `level` (the reference's silence
        clamp; passed unclamped through vocoder.vocode), averaged over the frames whose window lies wholly inside the waveform."""
        mel = torch.full((int(frames), N_MELS), float(level), dtype=torch.float32, device=self.device)
        w = vocoder.vocode([mel])[0].to(self.device, torch.float32).contiguous()
        n = int(w.numel())
        if n < MIN_SAMPLES:
            raise ValueError(f"the vocoder made {n} samples of a {frames}-frame mel; the bias needs at least {MIN_SAMPLES}")
        out = torch.empty(N_BINS, dtype=torch.float32, device=self.device)
        kk.call("kk_stft_mag_mean", w, n, 2, 1 + n // HOP - 2, self.tw, self.window, out)
        return self.set_bias(out)

    def tiles(self, samples: Sequence[int]) -> torch.Tensor:
        """int32 [ntiles, 2]: {utterance, first hop of the tile}; the tiles of an utterance cover its ceil(samples / 256) hops."""
        return torch.tensor([[b, f0] for b, n in enumerate(samples) for f0 in range(0, -(-n // HOP), self.tile_frames)], dtype=torch.int32)

    def denoise(self, waves: Sequence[torch.Tensor], strength: float = DEFAULT_STRENGTH) -> List[torch.Tensor]:
        """One fp32 waveform per input waveform [samples_b], in input order and of the same length.  strength 0 returns clones."""
        s = check_strength(strength)
        if self.bias is None:
            raise ValueError("SpectralDenoiser: no bias (set_bias or bias_from_vocoder first)")
        waves = list(waves)
        for i, w in enumerate(waves):
            if w.dim() != 1 or w.numel() < MIN_SAMPLES:
                raise ValueError(f"waveform {i}: shape {tuple(w.shape)}, expected [samples >= {MIN_SAMPLES}]: the STFT reflect-pads "
                                 f"{N_FFT // 2} samples at each end and the shortest vocoded utterance has {MIN_SAMPLES}")
        if s == 0.0:
            return [w.to(self.device, torch.float32).clone() for w in waves]
        if not waves:
            return []
        n = [int(w.numel()) for w in waves]
        x = torch.cat([w.to(self.device, torch.float32) for w in waves]).contiguous()
        woff = kk.packed_offsets(n, torch.int64, self.device)
        tiles = self.tiles(n).to(self.device)
        y = torch.empty_like(x)
        kk.call("kk_denoise", x, woff, tiles, tiles.shape[0], self.bias, s, self.tw, self.window, y)
        return list(y.split(n))
