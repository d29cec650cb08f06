"""The three prosody kernels (kk_prosody.hip) restated in fp32 torch, operation for operation: what the GPU tests compare against
with torch.equal, and what the tests' oracle puts into the reference's variance adaptor.  Runs anywhere; no GPU needed."""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def durations(d: torch.Tensor, speed: torch.Tensor, forced: torch.Tensor, plens: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """kk_prosody_durations.  d = expm1(log_dur) fp32 [B, Pn]; speed fp32 [B, Pn]; forced int [B, Pn], < 0 = not forced; plens [B] or
    None (every position counts).  Returns (dur int64 [B, Pn], row sums int64 [B])."""
    d, speed = d.to(torch.float32), speed.to(torch.float32)
    zero, one = torch.zeros((), dtype=torch.float32, device=d.device), torch.ones((), dtype=torch.float32, device=d.device)
    r = torch.round(d)                                                    # half to even
    s = torch.round(d / speed)                                            # tensor / tensor: an IEEE fp32 division per element
    scaled = torch.where(r > 0, torch.where(s > 1, s, one), zero).to(torch.int64)     # base == 0 (or NaN) -> 0, else >= 1 frame
    forced = forced.to(torch.int64)
    dur = torch.where(forced >= 0, forced, scaled)
    if plens is not None:
        Pn = d.shape[1]
        dur = torch.where(torch.arange(Pn, device=d.device)[None, :] < plens.to(torch.int64)[:, None], dur, torch.zeros_like(dur))
    return dur, dur.sum(dim=1)


def _scale_shift(c: torch.Tensor, s: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    m = c * s                                                             # two fp32 roundings: the kernel does not contract them
    return (m + b).clamp(0.0, 1.0)


def variance(pitch: torch.Tensor, energy: torch.Tensor, idx: torch.Tensor, lens: torch.Tensor, ps: torch.Tensor, pb: torch.Tensor,
             es: torch.Tensor, eb: torch.Tensor, fp: torch.Tensor, fe: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """kk_prosody_variance.  pitch, energy fp32 [B, T]; idx int64 [B, T] = the phoneme of every frame; lens [B] = frames per row; the
    six tables [B, Pn].  Returns the controlled (pitch, energy) [B, T]."""
    B, T = pitch.shape
    Pn = ps.shape[1]
    cp, ce = pitch.to(torch.float32).clamp(0.0, 1.0), energy.to(torch.float32).clamp(0.0, 1.0)
    live = (torch.arange(T, device=pitch.device)[None, :] < lens.to(torch.int64)[:, None]) & (idx >= 0) & (idx < Pn)
    j = idx.clamp(0, Pn - 1)
    g = lambda t: torch.gather(t.to(torch.float32), 1, j)
    fpj, fej = g(fp), g(fe)
    p = torch.where(~torch.isnan(fpj), fpj, torch.where(cp > 0, _scale_shift(cp, g(ps), g(pb)), cp))
    e = torch.where(~torch.isnan(fej), fej, _scale_shift(ce, g(es), g(eb)))
    return torch.where(live, p, cp), torch.where(live, e, ce)


def contour(pitch: torch.Tensor, energy: torch.Tensor, idx: torch.Tensor, lens: torch.Tensor, ps: torch.Tensor, pb: torch.Tensor,
            es: torch.Tensor, eb: torch.Tensor, fp: torch.Tensor, fe: torch.Tensor, dur: torch.Tensor, sd: torch.Tensor,
            pc: Optional[torch.Tensor], ec: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """kk_prosody_contour: variance() with a frame-level source track per row on top.  dur int [B, Pn] = the durations the frames
    were expanded by; sd int [B, Pn] >= 0 = the source frames of each phoneme; pc, ec fp32 [B, Sn] or None = the pitch / energy
    source tracks, NaN = not given at this frame.

    cs_t, cs_s = the exclusive prefix sums of dur and sd.  Frame t < lens[b] of phoneme j = idx[b, t]: n = dur[b, j], m = sd[b, j],
    k = t - cs_t[j], and when m > 0 the source frame s = cs_s[j] + (2k + 1) m // (2n) in int64: the centre-aligned nearest one, the
    identity when n == m.  Pitch: v = pc[b, s] not NaN -> v > 0 ? clamp(v * ps + pb, 0, 1) : v (an unvoiced source frame stays
    unvoiced); energy: v = ec[b, s] not NaN -> clamp(v * es + eb, 0, 1); everything else is variance()'s value.  Precedence: contour,
    per-phoneme forced value, the model.  s outside [0, Sn) (tables that do not fit the track) counts as not given."""
    B, T = pitch.shape
    Pn = ps.shape[1]
    p, e = variance(pitch, energy, idx, lens, ps, pb, es, eb, fp, fe)
    dev = pitch.device
    dur, sd = dur.to(torch.int64).clamp(min=0), sd.to(torch.int64).clamp(min=0)
    cs_t, cs_s = dur.cumsum(1) - dur, sd.cumsum(1) - sd
    t = torch.arange(T, device=dev, dtype=torch.int64)[None, :]
    live = (t < lens.to(torch.int64)[:, None]) & (idx >= 0) & (idx < Pn)
    j = idx.clamp(0, Pn - 1)
    n, m, k = torch.gather(dur, 1, j), torch.gather(sd, 1, j), t - torch.gather(cs_t, 1, j)
    s = torch.gather(cs_s, 1, j) + torch.div((2 * k + 1) * m, 2 * n.clamp(min=1), rounding_mode="floor")
    g = lambda tab: torch.gather(tab.to(torch.float32), 1, j)
    for which, track in (("p", pc), ("e", ec)):
        if track is None:
            continue
        Sn = track.shape[1]
        ok = live & (m > 0) & (n > 0) & (k >= 0) & (k < n) & (s >= 0) & (s < Sn)
        v = torch.gather(track.to(torch.float32), 1, s.clamp(0, max(Sn - 1, 0))) if Sn > 0 else torch.full_like(p, float("nan"))
        ok = ok & ~torch.isnan(v)
        if which == "p":
            p = torch.where(ok, torch.where(v > 0, _scale_shift(v, g(ps), g(pb)), v), p)
        else:
            e = torch.where(ok, _scale_shift(v, g(es), g(eb)), e)
    return p, e
