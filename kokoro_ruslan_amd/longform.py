"""Long-form synthesis on the device, on the kernels of csrc/kk_longform.hip: what the reference's text_to_speech does to every chunk
of a text between the model and the audio file (inference/inference.py:569-648).

`MelFinisher.finish` takes the mels of a batch, packed back to back, through one launch: the health statistics of the raw mel (NaN
count, min, max, mean, standard deviation), the clamp to [-11.5, 2] and the adaptive trailing-silence trim.  The one host read at the
end brings back the frame counts and the statistics; the trimmed mels are views of the clamped buffer and stay on the device, ready
for the vocoder.  `join` lays the chunk waveforms of any number of documents out back to back, with a gap of silence between the
chunks of one document, in one launch that also takes every chunk's peak (the reference's near-silence check).  Every row's results
equal, bit for bit, what it gets alone.  The definitions and their fp64 restatement: longform_torch.py."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.longform_torch import CLAMP, FLAT_STD, MARGIN, MAX_FRAMES, MIN_KEEP, THRESHOLD, check_documents, fade_table


def _pair(name: str, v) -> Tuple[float, float]:
    try:
        lo, hi = (float(a) for a in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (low, high) pair, not {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"{name} must be finite with low <= high, not {v!r}")
    return lo, hi


def _count(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v or v < 0:
        raise ValueError(f"{name} must be an integer >= 0, not {v!r}")
    return int(v)


class MelFinisher:
    """finish() on lists of mels [1 <= frames_b <= 4096, n_mels]: statistics, clamp and trailing-silence trim in one launch."""

    def __init__(self, device: str = "cuda", n_mels: int = 80, clamp: Tuple[float, float] = CLAMP,
                 threshold: Tuple[float, float] = THRESHOLD, margin: int = MARGIN, min_keep: int = MIN_KEEP):
        if isinstance(n_mels, bool) or int(n_mels) != n_mels or not 1 <= n_mels <= 128:
            raise ValueError(f"n_mels {n_mels!r}: expected an integer in [1, 128]")
        self.clamp, self.threshold = _pair("clamp", clamp), _pair("threshold", threshold)
        self.margin, self.min_keep = _count("margin", margin), _count("min_keep", min_keep)
        kk.load()
        self.device = torch.device(device)
        self.n_mels = int(n_mels)

    def finish(self, mels: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[Dict]]:
        """(trimmed, info) in input order: trimmed[b] = the clamped mel's first `kept` frames, fp32 on the device (a view of one
        buffer); info[b] = {"frames", "kept", "last_voiced" (-1: no frame above the threshold, nothing trimmed), "threshold", "min",
        "max", "mean", "std" (of the raw mel), "nan" (count), "flat" (std < 1e-5)}."""
        mels = list(mels)
        if not mels:
            return [], []
        for i, m in enumerate(mels):
            if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.shape[1] != self.n_mels or m.shape[0] < 1:
                raise ValueError(f"mel {i}: shape {tuple(getattr(m, 'shape', ()))}, expected [frames >= 1, {self.n_mels}]")
            if m.shape[0] > MAX_FRAMES:
                raise ValueError(f"mel {i}: {m.shape[0]} frames, the limit is {MAX_FRAMES}")
        T = [int(m.shape[0]) for m in mels]
        B, frames = len(T), sum(T)
        x = torch.cat([m.detach().to(self.device, torch.float32) for m in mels]).contiguous()
        moff = kk.packed_offsets(T, torch.int64, self.device)
        out = torch.empty_like(x)
        ends = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        stats = torch.empty(B, 6, dtype=torch.float64, device=self.device)
        kk.call("kk_mel_finish", x, moff, B, frames, self.n_mels, self.clamp[0], self.clamp[1], self.threshold[0], self.threshold[1],
                self.margin, self.min_keep, out, ends, stats)
        host = torch.cat([ends.to(torch.float64), stats], dim=1).cpu().tolist()      # the one host read (frame counts are exact in fp64)
        trimmed, info, off = [], [], 0
        for t, (t_end, last, thr, vmin, vmax, mean, std, nan) in zip(T, host):
            trimmed.append(out[off:off + int(t_end)])
            info.append({"frames": t, "kept": int(t_end), "last_voiced": int(last), "threshold": thr, "min": vmin, "max": vmax,
                         "mean": mean, "std": std, "nan": int(nan), "flat": bool(std < FLAT_STD)})
            off += t
        return trimmed, info


def join(waves: Sequence[torch.Tensor], documents: Sequence[Sequence[int]], gap: int, fade: int = 0, device: str = "cuda",
         out: Optional[torch.Tensor] = None) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """(docs, peaks): docs[d] = the waveforms documents[d] names, in that order, with `gap` zero samples between consecutive ones,
    fp32 on the device (views of one buffer); peaks fp32 [len(waves)] on the device = max |x| of every chunk.  fade > 0 multiplies the
    first and last min(fade, n / 2) samples of every chunk by a raised-cosine ramp (longform_torch.fade_table); 0 copies.  out: the buffer to build the
    documents in, a contiguous fp32 tensor on the device with exactly the samples of all documents; every one of them is written."""
    waves = list(waves)
    for i, w in enumerate(waves):
        if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() < 1:
            raise ValueError(f"waveform {i}: shape {tuple(getattr(w, 'shape', ()))}, expected [samples >= 1]")
    docs = check_documents(documents, len(waves))
    gap, fade = _count("gap", gap), _count("fade", fade)
    if not waves:
        return [], torch.zeros(0, dtype=torch.float32, device=device)
    kk.load()
    dev = torch.device(device)
    order = [c for d in docs for c in d]                                  # packed in playback order: dst ascends
    n = [int(waves[c].numel()) for c in order]
    dst, bounds, pos = [], [], 0
    for d in docs:
        start = pos
        for k, c in enumerate(d):
            pos += gap if k else 0
            dst.append(pos)
            pos += int(waves[c].numel())
        bounds.append((start, pos))
    total = pos
    if total >= 2 ** 31:
        raise ValueError(f"{total} output samples in the call: the kernel indexes fewer than 2^31; split the call")
    x = torch.cat([waves[c].detach().to(dev, torch.float32) for c in order]).contiguous()
    woff = kk.packed_offsets(n, torch.int64, dev)
    dst_t = torch.tensor(dst, dtype=torch.int64).to(dev)
    table = fade_table(fade).to(dev) if fade else None
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != (total,) or not out.is_contiguous():
        raise ValueError(f"out: {out.dtype} {tuple(out.shape)} on {out.device}, expected contiguous float32 ({total},) on {x.device}")
    peak = torch.empty(len(order), dtype=torch.float32, device=dev)
    kk.call("kk_wave_join", x, woff, dst_t, len(order), table, fade, total, out, peak)
    peaks = peak
    if order != sorted(order):                                            # back to the caller's chunk numbering
        peaks = torch.empty_like(peak)
        peaks[torch.tensor(order, dtype=torch.int64).to(dev)] = peak
    return [out[a:b] for a, b in bounds], peaks
