"""Free-running evaluation of a checkpoint: synthesize a set of utterances with the stop rule deciding, align every mel with its
ground truth by dynamic time warping on the device (kokoro_ruslan_amd.dtw) and report what teacher-forced validation cannot see:
MCD-DTW, the aligned mel L1, the length ratio, rows that ran into their generation bound, and the duration predictor's total error.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

METRICS = ("mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err")


def _generate(engine, ids, stress, stream: bool, slots: int, batch_size: int, controls: Dict[str, Any], prosody=None):
    """(mels, info) in input order: one generate_stream call, or synthesize()'s batches (sorted by phoneme count) of generate_batch.
    prosody: None, or one entry per utterance, handed to the engine with its utterance."""
    if stream:
        if slots < 1:
            raise ValueError("slots must be >= 1")
        if prosody is not None:
            controls = dict(controls, prosody=prosody)
        return engine.generate_stream(list(ids), list(stress) if stress is not None else None, slots=slots, want_info=True, **controls)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    N = len(ids)
    order = sorted(range(N), key=lambda i: (int(ids[i].numel()), i))
    mels: List[Optional[torch.Tensor]] = [None] * N
    info = {"durations": [None] * N, "T": [None] * N, "bounds": [None] * N}
    for s in range(0, N, batch_size):
        part = order[s:s + batch_size]
        kw = controls if prosody is None else dict(controls, prosody=[prosody[i] for i in part])
        m, inf = engine.generate_batch([ids[i] for i in part], [stress[i] for i in part] if stress is not None else None,
                                       want_info=True, **kw)
        for n, i in enumerate(part):
            mels[i] = m[n]
            for k in info:
                info[k][i] = inf[k][n]
    return mels, info


def summarize(records: Sequence[Dict]) -> Dict[str, Any]:
    """{"utterances", "hit_bound_share", metric: {"mean", "median", "p95"}} over the records (a metric no record has is left out)."""
    out: Dict[str, Any] = {"utterances": len(records),
                           "hit_bound_share": sum(bool(r["hit_bound"]) for r in records) / len(records) if records else 0.0}
    for k in METRICS:
        v = [float(r[k]) for r in records if k in r]
        if v:
            t = torch.tensor(v, dtype=torch.float64)
            out[k] = {"mean": float(t.mean()), "median": float(torch.quantile(t, 0.5)), "p95": float(torch.quantile(t, 0.95))}
    return out


def evaluate(engine, ids: Sequence[torch.Tensor], stress: Optional[Sequence[torch.Tensor]], ref_mels: Sequence[torch.Tensor], *,
             stream: bool = True, slots: int = 32, batch_size: int = 32, durations: Optional[Sequence[torch.Tensor]] = None,
             names: Optional[Sequence[str]] = None, mcep: int = 13, aligner=None, prosody=None,
             **controls) -> Tuple[List[Dict], Dict[str, Any]]:
    """Synthesize every utterance free-running (generate_stream with `slots` rows, or generate_batch `batch_size` at a time) and
    compare it with ref_mels[i] [frames, n_mels].  controls: the stop controls of generate_batch.  Returns (records, summary):
    per utterance {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw" (dB), "mel_l1_dtw", "hit_bound" (the row ended at its
    generation bound, not by the stop rule)} and, with ground-truth `durations`, "dur_abs_err" = |sum predicted - sum true| frames;
    summarize() of them.  prosody: one kokoro_ruslan_amd.prosody.Prosody for every utterance or one per utterance (None: no controls):
    with the ground-truth durations forced, dur_abs_err is 0 and the other metrics are the decoder's alone."""
    N = len(ids)
    if len(ref_mels) != N:
        raise ValueError(f"{len(ref_mels)} reference mels for {N} utterances")
    for what, v in (("stress", stress), ("durations", durations), ("names", names)):
        if v is not None and len(v) != N:
            raise ValueError(f"{what}: {len(v)} entries for {N} utterances")
    if N == 0:
        return [], summarize([])
    if prosody is not None:
        from kokoro_ruslan_amd.prosody import as_list
        prosody = as_list(prosody, N)
    mels, info = _generate(engine, ids, stress, stream, slots, batch_size, controls, prosody)
    if aligner is None:
        from kokoro_ruslan_amd.dtw import MelAligner
        aligner = MelAligner(device=engine.device, K=mcep)
    aligned = aligner.align(mels, ref_mels)
    records = []
    for i, (mel, al) in enumerate(zip(mels, aligned)):
        rec = {"name": names[i] if names is not None else i, "frames": int(mel.shape[0]), "ref_frames": int(ref_mels[i].shape[0]),
               "len_ratio": al["len_ratio"], "mcd_dtw": al["mcd_dtw"], "mel_l1_dtw": al["mel_l1_dtw"],
               "hit_bound": int(mel.shape[0]) >= int(info["bounds"][i][2])}
        if durations is not None:
            rec["dur_abs_err"] = abs(float(info["durations"][i].sum()) - float(durations[i].sum()))
        records.append(rec)
    return records, summarize(records)
