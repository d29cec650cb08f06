"""Audio feature extraction on the device: a batch of waveforms to log-mel, pitch and energy, on the kernels of csrc/kk_features.hip.

`FeatureExtractor` restates the acoustic half of the reference's dataset front-end (data/dataset.py:644-869) at its TrainingConfig
defaults: 22050 Hz, n_fft = win = 1024, hop 256, 80 HTK mels over 0-8000 Hz; PitchExtractor (YIN-style CMND, window 2048, 50-800 Hz)
and EnergyExtractor (log1p of the mean linear mel, 5 % / 95 % quantile scaling).  The waveforms of one call are packed back to back
with an offsets table and run through four launches: peak, mel, pitch, finish.  Every sum and every statistic of an utterance runs over
its own samples in a fixed order, so row b of a batch is, bit for bit, the utterance extracted alone.  All arithmetic is fp32, as in
the reference.  `extract_perturbed` puts the resampler (kokoro_ruslan_amd/resample.py) in front of the same four launches: the
reference's train-time speed perturbation.  The phonemizer and MFA alignment are not here.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.griffinlim import melscale_fbanks
from kokoro_ruslan_amd.stft import HOP, N_FFT, N_MELS, SAMPLE_RATE, device_tables

PITCH_WIN = 2048
DEFAULT_MAX_SAMPLES = 1 << 26           # packed samples per group (256 MB of fp32 waveform; a longer waveform runs alone)


def check_wave(i: int, w: torch.Tensor) -> None:
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or not w.dtype.is_floating_point:
        raise ValueError(f"waveform {i}: expected a 1-D float tensor of mono samples, got "
                         f"{tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}"
                         f"{' ' + str(w.dtype) if isinstance(w, torch.Tensor) else ''}")
    if w.shape[0] < 1:
        raise ValueError(f"waveform {i}: empty")
    if w.shape[0] >= 1 << 30:
        raise ValueError(f"waveform {i}: {w.shape[0]} samples; at most 2^30 - 1")


def mel_spans(fb: torch.Tensor) -> torch.Tensor:
    """int32 [80, 2]: the bins [lo, hi) where each column of the filterbank [513, 80] is non-zero (its triangle)."""
    rows = []
    for m in range(fb.shape[1]):
        nz = torch.nonzero(fb[:, m] > 0)[:, 0]
        rows.append([int(nz[0]), int(nz[-1]) + 1] if nz.numel() else [0, 0])
    return torch.tensor(rows, dtype=torch.int32)


class FeatureExtractor:
    """Batched feature extraction on the MI355X: extract(list of mono waveforms) -> per utterance mel_spec [80, T], pitch [T],
    energy [T], mel_length T = min(1 + max(n, 1024) // 256, max_seq_length)."""

    sampling_rate = SAMPLE_RATE
    hop = HOP

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        fb = melscale_fbanks(torch.float64)
        self.fb = fb.to(torch.float32).contiguous().to(self.device)
        self.span = mel_spans(fb).to(self.device)
        self.window, self.tw = device_tables(self.device)
        self.pitch_window = torch.hann_window(PITCH_WIN, periodic=True, dtype=torch.float64).to(torch.float32).to(self.device)
        self.tile_frames = int(kk.load().kk_feat_mel_tile_frames())
        self._resampler = None

    def extract(self, waves: Sequence[torch.Tensor], max_seq_length: int = 1800, variance: bool = True,
                max_samples: int = DEFAULT_MAX_SAMPLES, keep_linear: bool = False,
                intermediates: bool = False) -> List[Dict[str, object]]:
        """One dict per waveform (1-D float tensors of un-normalised mono samples at 22050 Hz, on any device), in input order:
        mel_spec [80, T], pitch [T], energy [T] (fp32, on the extractor's device) and mel_length.  variance=False gives zero pitch
        and energy.  The waveforms run in groups of at most max_samples packed samples.  keep_linear adds mel_linear [80, T];
        intermediates adds what the pitch kernel writes per pitch frame (pitch_candidate, pitch_acmax, pitch_msq)."""
        if int(max_seq_length) != max_seq_length or max_seq_length < 1:
            raise ValueError(f"max_seq_length must be an integer >= 1, not {max_seq_length!r}")
        if int(max_samples) != max_samples or max_samples < 1:
            raise ValueError(f"max_samples must be an integer >= 1, not {max_samples!r}")
        for i, w in enumerate(waves):
            check_wave(i, w)
        out: List[Dict[str, object]] = []
        group, total = [], 0
        for w in waves:
            if group and total + w.shape[0] > max_samples:
                out += self._run(group, int(max_seq_length), variance, keep_linear, intermediates)
                group, total = [], 0
            group.append(w)
            total += w.shape[0]
        if group:
            out += self._run(group, int(max_seq_length), variance, keep_linear, intermediates)
        return out

    def extract_perturbed(self, waves: Sequence[torch.Tensor], factors: Sequence[float], max_seq_length: int = 1800,
                          variance: bool = True, max_samples: int = DEFAULT_MAX_SAMPLES) -> List[Dict[str, object]]:
        """extract() of Resampler.speed_perturb(waves, factors), bit for bit, without the waveforms leaving the device in between: the
        reference's features of a speed-perturbed training sample (dataset.py:672-707).  Waveform b is peak-normalised, resampled
        22050 -> int(22050 factors[b]) and peak-normalised again, then runs through the four feature launches.  All lengths are
        computed on the host (ceil(n L / o) samples).  The waveforms run in groups of at most max_samples packed samples, counted
        before and after resampling."""
        from kokoro_ruslan_amd import resample as RS
        if int(max_seq_length) != max_seq_length or max_seq_length < 1:
            raise ValueError(f"max_seq_length must be an integer >= 1, not {max_seq_length!r}")
        if int(max_samples) != max_samples or max_samples < 1:
            raise ValueError(f"max_samples must be an integer >= 1, not {max_samples!r}")
        if len(factors) != len(waves):
            raise ValueError(f"{len(factors)} factors for {len(waves)} waveforms")
        for i, w in enumerate(waves):
            check_wave(i, w)
        if self._resampler is None:
            self._resampler = RS.Resampler(self.device)
        rows = [RS.rate_row(SAMPLE_RATE, RS.perturbed_rate(f, SAMPLE_RATE)) for f in factors]
        size = [max(int(w.shape[0]), RS.out_length(w.shape[0], r)) for w, r in zip(waves, rows)]
        out: List[Dict[str, object]] = []
        group, total = [], 0
        for i in list(range(len(waves))) + [None]:
            if group and (i is None or total + size[i] > max_samples):
                n = [int(waves[k].shape[0]) for k in group]
                pack = torch.cat([waves[k].to(self.device, torch.float32) for k in group]).contiguous()
                wave, m = self._resampler.run_packed(pack, n, [rows[k] for k in group], True)
                out += self._run_packed(wave, m, int(max_seq_length), variance, False, False)
                group, total = [], 0
            if i is not None:
                group.append(i)
                total += size[i]
        return out

    def _run(self, waves: List[torch.Tensor], max_T: int, variance: bool, keep_linear: bool, intermediates: bool):
        n = [int(w.shape[0]) for w in waves]
        wave = torch.cat([w.to(self.device, torch.float32) for w in waves]).contiguous()
        return self._run_packed(wave, n, max_T, variance, keep_linear, intermediates)

    def _run_packed(self, wave: torch.Tensor, n: List[int], max_T: int, variance: bool, keep_linear: bool, intermediates: bool):
        """wave: the fp32 waveforms of n[b] samples each, back to back on the device."""
        dev = self.device
        B = len(n)
        T = [min(1 + max(v, N_FFT) // HOP, max_T) for v in n]
        Tp = [1 + max(v, PITCH_WIN) // HOP for v in n]
        woff = kk.packed_offsets(n, torch.int64, dev)
        moff, poff = kk.packed_offsets(T, torch.int32, dev), kk.packed_offsets(Tp, torch.int32, dev)
        tiles = torch.tensor([[b, f0] for b, t in enumerate(T) for f0 in range(0, t, self.tile_frames)], dtype=torch.int32).to(dev)
        nm, npf = sum(T), sum(Tp)
        peak = torch.empty(B, dtype=torch.float32, device=dev)
        logmel = torch.empty(N_MELS * nm, dtype=torch.float32, device=dev)
        linmel = torch.empty(N_MELS * nm, dtype=torch.float32, device=dev) if keep_linear else None
        eraw = torch.empty(nm, dtype=torch.float32, device=dev)
        pitch = torch.empty(nm, dtype=torch.float32, device=dev)
        energy = torch.empty(nm, dtype=torch.float32, device=dev)
        kk.call("kk_feat_peak", wave, woff, B, max(n), peak)
        kk.call("kk_feat_mel", wave, woff, peak, moff, tiles, tiles.shape[0], self.tw, self.window, self.fb, self.span, logmel, linmel,
                eraw)
        ws = None
        if variance:
            frames = torch.stack([torch.repeat_interleave(torch.arange(B), torch.tensor(Tp)),
                                  torch.cat([torch.arange(t) for t in Tp])], 1).to(torch.int32).to(dev)
            ws = torch.empty(5, npf, dtype=torch.float32, device=dev)
            kk.call("kk_feat_pitch", wave, woff, peak, poff, frames, npf, self.pitch_window, ws[0], ws[1], ws[2])
            kk.call("kk_feat_finish", moff, poff, B, eraw, ws[0], ws[1], ws[2], ws[3], ws[4], pitch, energy, 1)
        else:
            kk.call("kk_feat_finish", moff, poff, B, eraw, None, None, None, None, None, pitch, energy, 0)
        mels = logmel.split([N_MELS * t for t in T])
        lins = linmel.split([N_MELS * t for t in T]) if keep_linear else None
        ps, es = pitch.split(T), energy.split(T)
        out = []
        for b in range(B):
            d = {"mel_spec": mels[b].view(N_MELS, T[b]), "pitch": ps[b], "energy": es[b], "mel_length": T[b]}
            if keep_linear:
                d["mel_linear"] = lins[b].view(N_MELS, T[b])
            out.append(d)
        if intermediates and variance:
            for b, (c, a, m) in enumerate(zip(ws[0].split(Tp), ws[1].split(Tp), ws[2].split(Tp))):
                out[b].update(pitch_candidate=c, pitch_acmax=a, pitch_msq=m)
        return out
