"""Edge trimming and loudness normalisation of waveforms on the device, on the kernels of csrc/kk_loudness.hip.

`LoudnessNormaliser` measures the ITU-R BS.1770-4 integrated loudness of mono waveforms (K-weighting, 400 ms blocks at 100 ms steps,
the absolute gate at -70 LUFS and the relative gate 10 LU under the ungated mean), trims leading and trailing silence by frame energy
against the loudest frame, and scales every waveform to a target loudness under a peak ceiling (the definitions and their constants:
loudness_torch.py, the fp64 restatement).  The waveforms of one call are packed back to back and run through at most five launches
with no host read between them; the one read at the end brings back {start, end} and the statistics.  Every sum runs in fp64 in an
order fixed by the sample's position in its own utterance, so an utterance's results do not depend on the rest of the batch.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.loudness_torch import FS_MAX, FS_MIN, HOP, block_sizes, kweight_coeffs

DEFAULT_TARGET, DEFAULT_PEAK_DB, DEFAULT_TOP_DB, DEFAULT_MARGIN_MS = -23.0, -1.0, 40.0, 50.0


def _finite(name: str, v: float) -> float:
    f = float(v)
    if not math.isfinite(f):
        raise ValueError(f"{name} must be finite, not {v!r}")
    return f


def check_top_db(top_db: float) -> float:
    t = _finite("top_db", top_db)
    if t <= 0:
        raise ValueError(f"top_db must be > 0, not {top_db!r}")
    return t


def check_peak_db(peak_db: float) -> float:
    p = _finite("peak_db", peak_db)
    if p > 0:
        raise ValueError(f"peak_db must be <= 0 (dB under full scale), not {peak_db!r}")
    return p


def check_margin_ms(margin_ms: float) -> float:
    m = _finite("margin_ms", margin_ms)
    if m < 0:
        raise ValueError(f"margin_ms must be >= 0, not {margin_ms!r}")
    return m


class LoudnessNormaliser:
    """measure / trim_edges / normalise on lists of mono waveforms [samples_b >= 1] at one sample rate in [8000, 48000]."""

    def __init__(self, device: str = "cuda", sample_rate: int = 22050):
        fs = int(sample_rate)
        if fs != sample_rate or not FS_MIN <= fs <= FS_MAX:
            raise ValueError(f"sample_rate {sample_rate!r}: expected an integer in [{FS_MIN}, {FS_MAX}]")
        kk.load()
        self.device = torch.device(device)
        self.sample_rate = fs
        self.block, self.step = block_sizes(fs)
        (b1, a1), (b2, a2) = kweight_coeffs(fs)
        self.coef = torch.tensor(b1 + a1[1:] + b2 + a2[1:], dtype=torch.float64).to(self.device)

    def _pack(self, waves: Sequence[torch.Tensor]):
        waves = list(waves)
        for i, w in enumerate(waves):
            if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() < 1:
                raise ValueError(f"waveform {i}: shape {tuple(getattr(w, 'shape', ()))}, expected [samples >= 1]")
        n = [int(w.numel()) for w in waves]
        if sum(n) >= 2 ** 31:
            raise ValueError(f"{sum(n)} samples in the batch: the kernels index fewer than 2^31; split the call")
        x = torch.cat([w.detach().to(self.device, torch.float32) for w in waves]).contiguous()
        woff = kk.packed_offsets(n, torch.int64, self.device)
        return n, x, woff

    def _offsets(self, n: Sequence[int], unit: int) -> Tuple[torch.Tensor, int]:
        off = kk.packed_offsets([-(-v // unit) for v in n])
        return off.to(torch.int32).to(self.device), int(off[-1])

    def _edges(self, n, x, woff, top_db: float, margin_ms: float) -> torch.Tensor:
        """int32 [B, 2] {start, end} on the device."""
        hoff, nhops = self._offsets(n, HOP)
        hopsq = torch.empty(nhops, dtype=torch.float64, device=self.device)
        se = torch.empty(len(n), 2, dtype=torch.int32, device=self.device)
        kk.call("kk_loud_hop_energy", x, woff, hoff, len(n), nhops, hopsq)
        kk.call("kk_loud_edges", hopsq, woff, hoff, len(n), top_db, int(round(margin_ms * self.sample_rate / 1000.0)), se)
        return se

    def _run(self, waves, target: float, peak_db: float, trim_db: Optional[float], margin_ms: float, apply: bool):
        n, x, woff = self._pack(waves)
        B = len(n)
        if trim_db is None:
            se = torch.tensor([[0, v] for v in n], dtype=torch.int32).to(self.device)
        else:
            se = self._edges(n, x, woff, trim_db, margin_ms)
        soff, nsteps = self._offsets(n, self.step)
        stepsq = torch.empty(nsteps, dtype=torch.float64, device=self.device)
        stepex = torch.empty(nsteps, dtype=torch.float64, device=self.device)
        steppk = torch.empty(nsteps, dtype=torch.float32, device=self.device)
        stats = torch.empty(B, 4, dtype=torch.float64, device=self.device)
        kk.call("kk_loud_kweight", x, woff, se, soff, B, nsteps, self.step, self.block, self.coef, stepsq, stepex, steppk)
        kk.call("kk_loud_gate", stepsq, stepex, steppk, se, soff, B, self.step, self.block, target, 10.0 ** (peak_db / 20.0), stats)
        y = None
        if apply:
            y = torch.empty_like(x)
            kk.call("kk_loud_apply", x, woff, se, stats, B, int(x.numel()), y)
        return n, y, se.cpu().tolist(), stats.cpu().tolist()               # the one host read

    def measure(self, waves: Sequence[torch.Tensor]) -> List[Optional[float]]:
        """Integrated loudness in LUFS per waveform; None where there is no block above the absolute gate (-inf)."""
        if not len(waves):
            return []
        _, _, _, stats = self._run(waves, DEFAULT_TARGET, 0.0, None, 0.0, apply=False)
        return [s[0] if s[0] > -math.inf else None for s in stats]

    def trim_edges(self, waves: Sequence[torch.Tensor], top_db: float = DEFAULT_TOP_DB,
                   margin_ms: float = DEFAULT_MARGIN_MS) -> List[Tuple[int, int]]:
        """(start, end) per waveform: what lies more than top_db under the loudest frame at either end is cut, margin_ms kept."""
        top_db, margin_ms = check_top_db(top_db), check_margin_ms(margin_ms)
        if not len(waves):
            return []
        n, x, woff = self._pack(waves)
        return [(int(s), int(e)) for s, e in self._edges(n, x, woff, top_db, margin_ms).cpu().tolist()]

    def normalise(self, waves: Sequence[torch.Tensor], target_lufs: float = DEFAULT_TARGET, peak_db: float = DEFAULT_PEAK_DB,
                  trim_db: Optional[float] = None, margin_ms: float = DEFAULT_MARGIN_MS) -> Tuple[List[torch.Tensor], List[Dict]]:
        """(waveforms x[start:end] * gain in fp32 and input order, info): info[b] = {"start", "end", "measured" (LUFS of the trimmed
        input, None for -inf), "gain", "limited"}.  trim_db None: no trim.  A waveform that measures -inf is left at gain 1."""
        target, peak_db, margin_ms = _finite("target_lufs", target_lufs), check_peak_db(peak_db), check_margin_ms(margin_ms)
        if trim_db is not None:
            trim_db = check_top_db(trim_db)
        if not len(waves):
            return [], []
        n, y, se, stats = self._run(waves, target, peak_db, trim_db, margin_ms, apply=True)
        out, info, off = [], [], 0
        for v, (s, e), st in zip(n, se, stats):
            out.append(y[off:off + e - s])
            info.append({"start": int(s), "end": int(e), "measured": st[0] if st[0] > -math.inf else None, "gain": float(st[1]),
                         "limited": bool(st[2])})
            off += v
        return out, info
