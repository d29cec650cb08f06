"""The last stretch of long-form synthesis in fp64 on the CPU: the yardstick the kernels of csrc/kk_longform.hip are tested and
benchmarked against (tests/test_longform_*.py, tools/longform_bench.py).  Not a fallback: kokoro_ruslan_amd.longform never calls it.

Finishing a mel [T >= 1, n_mels] (reference inference/inference.py:569-619):
  statistics of the RAW mel (:569-580): the number of NaNs, min and max over the values that are not NaN (+inf / -inf when there is
  none), the mean and the unbiased standard deviation (sum of squared deviations about the mean over T n_mels - 1; NaN when the mel
  holds a NaN or has one value).
  clamped = clamp(mel, lo, hi) (:588), a NaN kept.
  m_t = mean of clamped frame t.  q10, q20 = the 0.1 and 0.2 quantiles of m by torch.quantile's default definition: sort, position
  q (T - 1), linear interpolation between the two neighbours.  thr = max(thr_lo, min(thr_hi, (q10 + q20) / 2)) (:599); a mel that
  holds a NaN has NaN quantiles, and Python's max(lo, min(hi, nan)) is hi: thr = thr_hi.
  last_voiced = the last t with m_t > thr (a NaN mean is not), -1 when there is none; then t_end = T (:621), otherwise t_end =
  min(T, max(min_keep, min(T, last_voiced + margin + 1))) (:610-612).
finish_reference also returns two decision margins: the smallest |m_t - thr| over the frames, and the distance of the unclipped
(q10 + q20) / 2 from thr_lo and thr_hi (inf for a mel with a NaN).  A test input whose margins are well above the fp32 error of a
frame mean has the same decisions in fp32, on the host function and on the device.

Joining (:637-648): the chunks of a document in playback order with `gap` zeros between consecutive ones and none at the ends.  The
first and last min(F, n / 2) samples of a chunk of n samples are multiplied by fade[j] and fade[n - 1 - j]: one fp32 multiply, as the
kernel does, so the result is comparable bit for bit; F = 0 is the reference's plain concatenation.  fade_table(F)[i] = 0.5 - 0.5
cos(pi (i + 0.5) / F), computed in fp64 and rounded to fp32.  peaks[c] = max |x| of chunk c before the fade (:637)."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch

CLAMP, THRESHOLD, MARGIN, MIN_KEEP = (-11.5, 2.0), (-9.8, -9.2), 24, 60
MAX_FRAMES = 4096         # of one mel: the kernel sorts its frame means in LDS
FLAT_STD, SILENT_PEAK = 1e-5, 1e-4       # the reference's warnings (:579, :639)


def quantile_linear(sorted_values: torch.Tensor, q: float) -> float:
    n = int(sorted_values.numel())
    pos = q * (n - 1)
    i0 = int(math.floor(pos))
    i1 = min(i0 + 1, n - 1)
    a, b = float(sorted_values[i0]), float(sorted_values[i1])
    return a + (pos - i0) * (b - a)


def finish_reference(mel: torch.Tensor, clamp: Tuple[float, float] = CLAMP, threshold: Tuple[float, float] = THRESHOLD,
                     margin: int = MARGIN, min_keep: int = MIN_KEEP):
    """(clamped fp32 [T, n_mels], t_end, last_voiced, thr, stats) of one fp32 mel [T >= 1, n_mels]; stats = {"min", "max", "mean",
    "std", "nan", "frame_margin", "branch_margin"}."""
    if mel.dim() != 2 or mel.shape[0] < 1 or mel.shape[1] < 1:
        raise ValueError(f"mel: shape {tuple(mel.shape)}, expected [frames >= 1, n_mels >= 1]")
    raw = mel.detach().cpu().to(torch.float32)
    T = int(raw.shape[0])
    x = raw.to(torch.float64)
    isnan = torch.isnan(x)
    nan = int(isnan.sum())
    good = x[~isnan]
    vmin = float(good.min()) if good.numel() else math.inf
    vmax = float(good.max()) if good.numel() else -math.inf
    mean = float(x.sum() / x.numel())
    std = float(((x - mean) ** 2).sum() / (x.numel() - 1)) ** 0.5 if x.numel() > 1 else math.nan
    clamped = torch.clamp(raw, min=clamp[0], max=clamp[1])
    m = clamped.to(torch.float64).mean(dim=-1)
    branch_margin = math.inf
    if nan:
        thr = float(threshold[1])
    else:
        s = torch.sort(m).values
        mid = 0.5 * (quantile_linear(s, 0.10) + quantile_linear(s, 0.20))
        thr = max(float(threshold[0]), min(float(threshold[1]), mid))
        branch_margin = min(abs(mid - threshold[0]), abs(mid - threshold[1]))
    voiced = (m > thr).nonzero().reshape(-1)
    last_voiced = int(voiced[-1]) if voiced.numel() else -1
    t_end = T if last_voiced < 0 else min(T, max(int(min_keep), min(T, last_voiced + int(margin) + 1)))
    dist = (m - thr).abs()
    dist = dist[~torch.isnan(dist)]
    stats = {"min": vmin, "max": vmax, "mean": mean, "std": std, "nan": nan,
             "frame_margin": float(dist.min()) if dist.numel() else math.inf, "branch_margin": branch_margin}
    return clamped, t_end, last_voiced, thr, stats


def fade_table(F: int) -> torch.Tensor:
    """fp32 [F]: the rising half of a raised cosine at the midpoints of its F steps."""
    i = torch.arange(int(F), dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(math.pi * (i + 0.5) / max(int(F), 1))).to(torch.float32)


def check_documents(documents: Sequence[Sequence[int]], chunks: int) -> List[List[int]]:
    """documents as lists of ints, checked: no empty document, every chunk index in [0, chunks) exactly once."""
    docs = [[int(c) for c in d] for d in documents]
    for k, d in enumerate(docs):
        if not d:
            raise ValueError(f"documents[{k}] is empty: a document needs at least one chunk")
    seen = sorted(c for d in docs for c in d)
    if seen != list(range(chunks)):
        raise ValueError(f"documents {docs!r}: every chunk index in [0, {chunks}) must appear exactly once")
    return docs


def join_reference(chunks: Sequence[torch.Tensor], documents: Sequence[Sequence[int]], gap: int, fade: int = 0):
    """(one fp32 waveform per document, peaks fp32 [C]) from chunk waveforms [samples_c >= 1] on the CPU."""
    chunks = [c.detach().cpu().to(torch.float32).reshape(-1) for c in chunks]
    docs = check_documents(documents, len(chunks))
    if int(gap) != gap or gap < 0 or int(fade) != fade or fade < 0:
        raise ValueError(f"gap {gap!r} and fade {fade!r} must be integers >= 0")
    table = fade_table(fade)
    silence = torch.zeros(int(gap), dtype=torch.float32)
    waves = []
    for d in docs:
        parts = []
        for k, c in enumerate(d):
            x = chunks[c].clone()
            nf = min(int(fade), x.numel() // 2)
            if nf:
                x[:nf] = x[:nf] * table[:nf]
                x[x.numel() - nf:] = x[x.numel() - nf:] * table[:nf].flip(0)
            if k:
                parts.append(silence)
            parts.append(x)
        waves.append(torch.cat(parts))
    peaks = torch.stack([c.abs().max() for c in chunks]) if chunks else torch.zeros(0)
    return waves, peaks
