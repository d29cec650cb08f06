"""Band-limited resampling on the device: a batch of waveforms, each with its own rate pair, on the kernel of csrc/kk_resample.hip.

`Resampler.resample` is `torchaudio.functional.resample` at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), pinned
to that method's definition (resample_torch) rather than to a run of torchaudio; `speed_perturb` is the reference's train-time
augmentation around it (data/dataset.py:672-684): peak-normalise, resample 22050 -> int(22050 f), peak-normalise.  The waveforms of
one call are packed back to back and run through one launch (four with the normalisations: peak, resample, peak, scale).  Every output
sample is a sum over its own utterance's samples in a fixed order, so row b of a batch is, bit for bit, the utterance resampled alone.
"""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple, Union

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.features import DEFAULT_MAX_SAMPLES, check_wave
from kokoro_ruslan_amd.resample_torch import rate_pair

SAMPLE_RATE = 22050
Rates = Union[int, Sequence[int]]


def _f32_bits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", v))[0]


def rate_row(orig_freq: int, new_freq: int) -> List[int]:
    """The kernel's per-utterance table row: {o, n, width, bits of fp32(base / (o n)), bits of fp32(base / o), 0, 0, 0}; equal rates
    give the copy row {1, 1, 0, 0, bits of 1.0}."""
    if int(orig_freq) == int(new_freq):
        rate_pair(orig_freq, new_freq)
        return [1, 1, 0, 0, _f32_bits(1.0), 0, 0, 0]
    o, n, base, width = rate_pair(orig_freq, new_freq)
    if not kk.load().kk_resample_supported(o, n, width):
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz ({o}:{n}) is outside the kernel's range: it takes down-sampling by up "
                         f"to about 14x")
    return [o, n, width, _f32_bits(base / (o * n)), _f32_bits(base / o), 0, 0, 0]


def out_length(length: int, row: List[int]) -> int:
    """ceil(n L / o)."""
    return (row[1] * int(length) + row[0] - 1) // row[0]


def _per_row(v: Rates, B: int, what: str) -> List[int]:
    if isinstance(v, (int, float)) or (isinstance(v, torch.Tensor) and v.dim() == 0):
        v = [v] * B
    v = [x.item() if isinstance(x, torch.Tensor) else x for x in v]
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} values for {B} waveforms")
    for i, x in enumerate(v):
        if int(x) != x or x < 1:
            raise ValueError(f"{what}[{i}]: a sample rate must be a positive integer, not {x!r}")
    return [int(x) for x in v]


def perturbed_rate(factor: float, sample_rate: int = SAMPLE_RATE) -> int:
    """int(sample_rate * factor), the reference's new_sr (dataset.py:681)."""
    if not (isinstance(factor, (int, float)) and 0.1 <= factor <= 10.0):
        raise ValueError(f"speed factor must be a number in [0.1, 10], not {factor!r}")
    return int(sample_rate * factor)


class Resampler:
    """Batched sinc resampling on the MI355X: resample(list of mono waveforms, orig_freq, new_freq) -> list of 1-D fp32 tensors of
    ceil(n L / o) samples each."""

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        self.tile = int(kk.load().kk_resample_tile())

    def resample(self, waves: Sequence[torch.Tensor], orig_freq: Rates, new_freq: Rates, normalise: bool = False,
                 max_samples: int = DEFAULT_MAX_SAMPLES) -> List[torch.Tensor]:
        """waves: 1-D float tensors of mono samples, on any device; orig_freq / new_freq: one int for all, or one per waveform.
        Returns fp32 tensors on the resampler's device, in input order.  A waveform whose rates are equal comes back unchanged, as from
        torchaudio.  normalise=True divides every waveform by (its peak + 1e-9) before and after (equal rates included).  The
        waveforms run in groups of at most max_samples packed input samples."""
        B = len(waves)
        for i, w in enumerate(waves):
            check_wave(i, w)
        if int(max_samples) != max_samples or max_samples < 1:
            raise ValueError(f"max_samples must be an integer >= 1, not {max_samples!r}")
        of, nf = _per_row(orig_freq, B, "orig_freq"), _per_row(new_freq, B, "new_freq")
        rows = [rate_row(a, b) for a, b in zip(of, nf)]
        for i, (w, r) in enumerate(zip(waves, rows)):
            if out_length(w.shape[0], r) >= 1 << 31:
                raise ValueError(f"waveform {i}: {out_length(w.shape[0], r)} output samples; at most 2^31 - 1")
        out: List[torch.Tensor] = [None] * B
        run = [i for i in range(B) if normalise or of[i] != nf[i]]
        for i in range(B):
            if out[i] is None and i not in run:
                out[i] = waves[i]
        group, total = [], 0
        for i in run + [None]:
            if group and (i is None or total + waves[i].shape[0] > max_samples):
                n = [int(waves[k].shape[0]) for k in group]
                pack = torch.cat([waves[k].to(self.device, torch.float32) for k in group]).contiguous()
                res, m = self.run_packed(pack, n, [rows[k] for k in group], normalise)
                for k, y in zip(group, res.split(m)):
                    out[k] = y
                group, total = [], 0
            if i is not None:
                group.append(i)
                total += waves[i].shape[0]
        return out

    def speed_perturb(self, waves: Sequence[torch.Tensor], factors: Sequence[float], sample_rate: int = SAMPLE_RATE,
                      max_samples: int = DEFAULT_MAX_SAMPLES) -> List[torch.Tensor]:
        """The reference's speed perturbation (dataset.py:672-684): x / (peak + 1e-9), resampled sample_rate -> int(sample_rate f),
        divided by (its new peak + 1e-9).  f > 1 gives a shorter, higher utterance."""
        if len(factors) != len(waves):
            raise ValueError(f"{len(factors)} factors for {len(waves)} waveforms")
        return self.resample(waves, sample_rate, [perturbed_rate(f, sample_rate) for f in factors], True, max_samples)

    def run_packed(self, wave: torch.Tensor, n: List[int], rows: List[List[int]], normalise: bool) -> Tuple[torch.Tensor, List[int]]:
        """One group on the device: wave = the fp32 waveforms of n[b] samples back to back, rows = rate_row per utterance.  Returns
        (the resampled waveforms back to back, their lengths); nothing comes back to the host in between."""
        dev, B = self.device, len(n)
        m = [out_length(v, r) for v, r in zip(n, rows)]
        woff_in, woff_out = kk.packed_offsets(n, torch.int64, dev), kk.packed_offsets(m, torch.int64, dev)
        rate = torch.tensor(rows, dtype=torch.int32).to(dev)
        tiles = torch.tensor([[b, j0] for b, v in enumerate(m) for j0 in range(0, v, self.tile)], dtype=torch.int32).to(dev)
        out = torch.empty(sum(m), dtype=torch.float32, device=dev)
        peak = None
        if normalise:
            peak = torch.empty(B, dtype=torch.float32, device=dev)
            kk.call("kk_feat_peak", wave, woff_in, B, max(n), peak)
        kk.call("kk_resample", wave, woff_in, peak, rate, tiles, tiles.shape[0], woff_out, out)
        if normalise:
            peak2 = torch.empty(B, dtype=torch.float32, device=dev)
            kk.call("kk_feat_peak", out, woff_out, B, max(m), peak2)
            kk.call("kk_resample_normalise", out, woff_out, B, max(m), peak2)
        return out, m
