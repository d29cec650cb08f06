"""What the contour tests share: the definition of kk_prosody_contour as a naive per-frame Python loop (written from the entry
point's comment in include/kokoro_hip.h, not from prosody_torch.contour), and the builder of the kernel tests' inputs."""
import math

import torch

NAN = math.nan


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def _clamp01(x):
    return x.clamp(0.0, 1.0)


def _scale_shift(v, s, b):
    m = _f32(v) * _f32(s)                                  # one fp32 product, then one fp32 sum
    return _clamp01(m + _f32(b))


def naive_contour(pitch, energy, idx, lens, ps, pb, es, eb, fp, fe, dur, sd, pc, ec):
    """Frame by frame, in Python integers and 0-d fp32 tensors.  Returns (pitch_out, energy_out) fp32 [B, T]."""
    B, T = pitch.shape
    Pn = ps.shape[1]
    out_p, out_e = torch.empty(B, T), torch.empty(B, T)
    for b in range(B):
        d, m_all = [max(int(x), 0) for x in dur[b]], [int(x) for x in sd[b]]
        cs_t = [sum(d[:j]) for j in range(Pn)]
        cs_s = [sum(m_all[:j]) for j in range(Pn)]
        for t in range(T):
            cp, ce = _clamp01(pitch[b, t].float()), _clamp01(energy[b, t].float())
            j = int(idx[b, t])
            if t >= int(lens[b]) or not 0 <= j < Pn:
                out_p[b, t], out_e[b, t] = cp, ce
                continue
            # today's rule: forced, else scaled and shifted
            p = fp[b, j] if not math.isnan(float(fp[b, j])) else (_scale_shift(cp, ps[b, j], pb[b, j]) if float(cp) > 0 else cp)
            e = fe[b, j] if not math.isnan(float(fe[b, j])) else _scale_shift(ce, es[b, j], eb[b, j])
            n, m, k = d[j], m_all[j], t - cs_t[j]
            if m > 0:
                assert 0 <= k < n, "idx and dur belong together"
                s = cs_s[j] + ((2 * k + 1) * m) // (2 * n)
                if pc is not None and s < pc.shape[1] and not math.isnan(float(pc[b, s])):
                    v = pc[b, s]
                    p = _scale_shift(v, ps[b, j], pb[b, j]) if float(v) > 0 else v
                if ec is not None and s < ec.shape[1] and not math.isnan(float(ec[b, s])):
                    e = _scale_shift(ec[b, s], es[b, j], eb[b, j])
            out_p[b, t], out_e[b, t] = p, e
    return out_p, out_e


def frames_of(dur, T):
    """(idx int64 [B, T], lens int64 [B]) as kk_length_regulate_index writes them for durations dur [B, Pn]: -1 past a row's frames."""
    B, Pn = dur.shape
    idx = torch.full((B, T), -1, dtype=torch.int64)
    lens = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        fr = torch.repeat_interleave(torch.arange(Pn), dur[b].clamp(min=0))[:T]
        idx[b, :fr.numel()] = fr
        lens[b] = fr.numel()
    return idx, lens


def kernel_inputs(Pn, seed, B=3):
    """The fourteen inputs of kk_prosody_contour for B = 3 rows of Pn phonemes with durations and source durations drawn from
    0..3 independently (so every ratio n : m of 0..3 occurs, zero-length phonemes on either side included) and ragged lens.
    Row 0 has no contour (sd = 0, tracks NaN), row 1 a pitch track only, row 2 both tracks with NaN holes.  T = the longest row plus
    a few frames and no multiple of 64.  The tracks hold exact zeros (unvoiced) among values in (0, 1]."""
    g = torch.Generator().manual_seed(seed)
    dur = torch.randint(0, 4, (B, Pn), generator=g)
    sd = torch.randint(0, 4, (B, Pn), generator=g).to(torch.int32)
    if Pn >= 4:                                                    # at fixed places, whatever the draw
        for b in range(B):
            dur[b, 0], sd[b, 0] = 0, 2                             # no frames, source frames
            dur[b, 1], sd[b, 1] = 3, 0                             # frames, no source frames
            dur[b, 2], sd[b, 2] = 3, 1                             # n = 3m
            dur[b, 3], sd[b, 3] = 1, 3                             # m = 3n
    else:
        dur[:, 0] = torch.tensor([2, 1, 3])[:B]
        sd[:, 0] = torch.tensor([2, 3, 1], dtype=torch.int32)[:B]
    dur[0, Pn // 2:] = 0                                           # row 0 is the shortest by far: ragged lens
    sd[0] = 0
    if Pn >= 4 and int(dur[1].sum()) == int(dur[2].sum()):         # three different lens, whatever the draw
        dur[2, -1] = (dur[2, -1] + 1) % 4
    T =max(int(dur.sum(dim=1).max()), 3) + 5
    T += 1 if T % 64 == 0 else 0
    idx, lens = frames_of(dur, T)
    Sn = max(int(sd.sum(dim=1).max()), 1)
    pitch = (torch.randn(B, T, generator=g) * 0.6 + 0.4).float()
    energy = (torch.randn(B, T, generator=g) * 0.6 + 0.5).float()
    pitch[:, 0], energy[:, 0] = 0.0, 1.0
    ps, es = 2.0 * torch.rand(B, Pn, generator=g), 2.0 * torch.rand(B, Pn, generator=g)
    pb, eb = torch.rand(B, Pn, generator=g) - 0.5, torch.rand(B, Pn, generator=g) - 0.5
    nan = torch.tensor(NAN)
    fp = torch.where(torch.rand(B, Pn, generator=g) < 0.3, torch.rand(B, Pn, generator=g), nan)
    fe = torch.where(torch.rand(B, Pn, generator=g) < 0.3, torch.rand(B, Pn, generator=g), nan)
    pc, ec = torch.rand(B, Sn, generator=g), torch.rand(B, Sn, generator=g)
    pc = torch.where(torch.rand(B, Sn, generator=g) < 0.25, torch.zeros(()), pc)         # unvoiced source frames
    pc[2] = torch.where(torch.rand(Sn, generator=g) < 0.2, nan, pc[2])
    ec[2] = torch.where(torch.rand(Sn, generator=g) < 0.2, nan, ec[2])
    pc[0], ec[0], ec[1] = NAN, NAN, NAN
    for b in range(B):                                             # past the row's own source frames: padding
        n = int(sd[b].sum())
        pc[b, n:], ec[b, n:] = NAN, NAN
    return pitch, energy, idx, lens, ps, pb, es, eb, fp, fe, dur.to(torch.int64), sd, pc.contiguous(), ec.contiguous()
