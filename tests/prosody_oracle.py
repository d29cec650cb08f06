"""The oracle of the prosody tests: oracle.kokoro_oracle.encode_for_inference restated with the controls put in at the two places the
engine puts them (prosody_torch.durations behind the duration predictor, prosody_torch.variance in front of the bucketize), built
from the oracle's own blocks.  generate() runs O.generate on that restatement by monkeypatching the module attribute; oracle/ itself
is left as it is.  A helper module, not a test file."""
import torch
import torch.nn.functional as F

from kokoro_ruslan_amd import prosody_torch as PT
from kokoro_ruslan_amd.prosody import pack
from oracle import kokoro_oracle as O

VA = "duration_adaptor.variance_adaptor"


def encode_for_inference(P, Bf, ids, stress, d, prosody):
    """O.encode_for_inference (B = 1, or a padded batch) under `prosody`: one Prosody or None per row, over all Pn positions.  The
    returned dict has the oracle's entries and "d" (expm1(log_dur)), "speed", "pitch_c" / "energy_c" (the controlled values that are
    bucketized), "pidx" / "eidx" (the buckets) and "live" (frames below the row's length)."""
    H = d.hidden
    pe = Bf["positional_encoding.pe"][0]
    B, Pn = ids.shape
    t = pack(list(prosody), [Pn] * B, Pn)
    text_mask = ids == 0
    x = F.embedding(ids, P["text_embedding.weight"]) * (H ** 0.5)
    if stress is not None:
        x = x + F.embedding(stress, P["stress_embedding.weight"], padding_idx=0)
    x = x + pe[:Pn]
    for i in range(d.enc_layers):
        x = O.encoder_block(P, i, x, text_mask, d.heads)
    enc = O._ln(P, "encoder_norm", x)
    log_dur = O.variance_predictor(P, f"{VA}.duration_predictor", enc, text_mask)
    dd = torch.expm1(log_dur)
    dur, sums = PT.durations(dd, t.speed, t.durations)
    xf = O.length_regulate(enc, dur, None)
    idx, _, _ = O.length_regulate_index(dur.numpy(), None)
    idx = torch.from_numpy(idx)
    if xf.size(1) < 3:
        idx = F.pad(idx, (0, 3 - xf.size(1)), value=-1)
        xf = F.pad(xf, (0, 0, 0, 3 - xf.size(1)))
    lengths = dur.sum(dim=1)
    Lp = xf.size(1)
    frame_mask = torch.arange(Lp).unsqueeze(0) >= lengths.unsqueeze(1)
    pitch = O.variance_predictor(P, f"{VA}.pitch_predictor", xf, frame_mask)
    energy = O.variance_predictor(P, f"{VA}.energy_predictor", xf, frame_mask)
    pc, ec = PT.variance(pitch, energy, idx, lengths, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy)
    pb = torch.bucketize(pc, Bf[f"{VA}.pitch_bins"])
    eb = torch.bucketize(ec, Bf[f"{VA}.energy_bins"])
    memory = xf + F.embedding(pb, P[f"{VA}.pitch_embedding.weight"]) + F.embedding(eb, P[f"{VA}.energy_embedding.weight"])
    memory = memory.masked_fill(frame_mask.unsqueeze(-1), 0.0)
    return {"memory": memory, "mem_mask": frame_mask, "log_dur": log_dur, "durations": dur, "pitch": pitch, "energy": energy, "enc": enc,
            "d": dd, "speed": t.speed, "pitch_c": pc, "energy_c": ec, "pidx": pb, "eidx": eb, "live": ~frame_mask}


def generate(monkeypatch, P, Bf, ids, stress, d, prosody, **kw):
    """O.generate(want=True) with encode_for_inference replaced by the restatement above under `prosody` (a list, one per row)."""
    with monkeypatch.context() as m:
        m.setattr(O, "encode_for_inference", lambda P_, Bf_, ids_, stress_, d_: encode_for_inference(P_, Bf_, ids_, stress_, d_, prosody))
        return O.generate(P, Bf, ids, stress, d, want=True, **kw)


def half_margin(d: torch.Tensor, speed: torch.Tensor) -> float:
    """The least distance of d and d / speed from a rounding boundary (k + 0.5) over the phonemes."""
    q = torch.cat([d.double().reshape(-1), (d.double() / speed.double()).reshape(-1)])
    return float(((q - torch.floor(q)) - 0.5).abs().min())


def bin_margin(values: torch.Tensor, live: torch.Tensor, bins: torch.Tensor) -> float:
    """The least distance of the live frames' values from a bin edge; exact zeros (clamped, or unvoiced pitch) are left out: they are
    the same exact value on both sides."""
    v = values[live & (values != 0)].double()
    if v.numel() == 0:
        return float("inf")
    return float((v[:, None] - bins.double()[None, :]).abs().min())

