"""Free-running evaluation of a checkpoint: synthesize a set of utterances with the stop rule deciding, align every mel with its
ground truth by dynamic time warping on the device (kokoro_ruslan_amd.dtw) and report what teacher-forced validation cannot see:
MCD-DTW, the aligned mel L1, the length ratio, rows that ran into their generation bound, and the duration predictor's total error.
With a vocoder the judgement goes on to the audio: every mel is vocoded (and denoised), the pitch and energy tracks of the waveforms
are extracted on the device (kokoro_ruslan_amd.features) and compared with the ground truth's along the same alignment: the F0 error
in cents, the voicing decision error, the gross pitch errors and the energy error.  With the speaker's recordings (ref_waves) the
waveforms are also held against them along that alignment (kokoro_ruslan_amd.spectral): spectral convergence, level offset and
log-spectral distance at three analysis windows, the numbers that move with the vocoder, the denoiser and Griffin-Lim's iterations.
evaluate_vocoder is the same judgement of the audio stage alone: the cache's own mels vocoded and compared with the recordings.
With a phone model (kokoro_ruslan_amd.align) the mels are also scored against the phonemes that were requested: goodness of
pronunciation, log posterior and frame accuracy of the synthesis, of the recording, and the gap between them.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

TRACK_METRICS = ("f0_rmse_cents", "f0_bias_cents", "gpe", "vuv_err", "energy_l1_dtw")
TRACK_COUNTS = ("n_vv", "n_vu", "n_uv", "n_uu", "n_gpe")
SPECTRAL_METRICS = ("mr_sc_dtw", "mr_lsd_dtw") + tuple(f"{k}_{w}" for w in (256, 512, 1024) for k in ("sc_dtw", "lsd_dtw", "level_db"))
SPECTRAL_COUNTS = ("spec_steps", "spec_skipped")
PRON_FIELDS = ("gop", "logpost", "phone_acc", "gop_min", "gop_min_token")     # of a PhoneAligner.score record
PRON_METRICS = ("gop", "logpost", "phone_acc", "gop_min", "ref_gop", "ref_logpost", "ref_phone_acc", "gop_gap", "phone_acc_gap")
METRICS = ("mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err") + TRACK_METRICS + SPECTRAL_METRICS + PRON_METRICS


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
    """{"utterances", "hit_bound_share", metric: {"mean", "median", "p95"}} over the records (a metric no record has is left out, a
    record whose value is None does not count: an F0 error without a step voiced on both sides).  Records of an evaluation with a
    vocoder carry "no_variance"; the summary then counts those that are (a cache written without pitch and energy)."""
    out: Dict[str, Any] = {"utterances": len(records),
                           "hit_bound_share": sum(bool(r.get("hit_bound")) for r in records) / len(records) if records else 0.0}
    for k in METRICS:
        v = [float(r[k]) for r in records if r.get(k) is not None]
        if v:
            t = torch.tensor(v, dtype=torch.float64)
            out[k] = {"mean": float(t.mean()), "median": float(torch.quantile(t, 0.5)), "p95": float(torch.quantile(t, 0.95))}
    if any("no_variance" in r for r in records):
        out["no_variance"] = sum(bool(r.get("no_variance")) for r in records)
    if any("gop_gap" in r for r in records):
        out["pron_infeasible"] = sum(r.get("gop_gap") is None for r in records)
    return out


def _pron_records(phone_aligner, phone_model, optional_ids, device, mels, ref_mels, ids) -> List[Dict]:
    """The pronunciation fields of every utterance: the synthesized mels and the recordings' scored against the requested phonemes."""
    if phone_aligner is None:
        from kokoro_ruslan_amd.align import PhoneAligner
        phone_aligner = PhoneAligner(device=device, K=int(phone_model["K"]), n_classes=int(phone_model["n_classes"]),
                                     states=int(phone_model.get("states", 1)), mixtures=int(phone_model.get("mixtures", 1)))
    syn = phone_aligner.score(list(mels), list(ids), optional_ids, phone_model)
    ref = phone_aligner.score(list(ref_mels), list(ids), optional_ids, phone_model)
    out = []
    for s, r in zip(syn, ref):
        rec = {k: s[k] for k in PRON_FIELDS}
        rec.update({f"ref_{k}": r[k] for k in ("gop", "logpost", "phone_acc")})
        both = s["feasible"] and r["feasible"]
        rec["gop_gap"] = s["gop"] - r["gop"] if both else None
        rec["phone_acc_gap"] = s["phone_acc"] - r["phone_acc"] if both else None
        out.append(rec)
    return out


def _check_audio_args(N: int, vocoder, vocoder_kwargs, denoiser, denoise_strength, extractor, ref_pitch, ref_energy, want_audio,
                      ref_waves=None, spectral=None) -> None:
    if vocoder is None:
        for what, v in (("vocoder_kwargs", vocoder_kwargs), ("denoiser", denoiser), ("extractor", extractor), ("ref_pitch", ref_pitch),
                        ("ref_energy", ref_energy), ("ref_waves", ref_waves), ("spectral", spectral)):
            if v is not None:
                raise ValueError(f"{what} needs a vocoder: it bears on the audio metrics alone")
        if want_audio:
            raise ValueError("want_audio needs a vocoder")
        return
    if ref_pitch is None or ref_energy is None:
        raise ValueError("a vocoder needs ref_pitch and ref_energy: the audio metrics compare against the ground truth's tracks")
    for what, v in (("ref_pitch", ref_pitch), ("ref_energy", ref_energy)):
        if len(v) != N:
            raise ValueError(f"{what}: {len(v)} entries for {N} utterances")
    if vocoder_kwargs is not None and not isinstance(vocoder_kwargs, dict):
        raise ValueError("vocoder_kwargs must be a dict of keyword arguments for the vocoder's vocode()")
    if denoiser is not None and not (isinstance(denoise_strength, (int, float)) and math.isfinite(denoise_strength) and denoise_strength >= 0):
        raise ValueError(f"denoise_strength must be a finite number >= 0, not {denoise_strength!r}")
    _check_ref_waves(N, ref_waves, spectral)


def _check_ref_waves(N: int, ref_waves, spectral) -> None:
    if ref_waves is None:
        if spectral is not None:
            raise ValueError("spectral needs ref_waves: it measures the audio against the recordings")
        return
    if len(ref_waves) != N:
        raise ValueError(f"ref_waves: {len(ref_waves)} entries for {N} utterances")
    for i, w in enumerate(ref_waves):
        if not isinstance(w, torch.Tensor) or w.dim() != 1 or not w.is_floating_point():
            raise ValueError(f"ref_waves[{i}] must be a 1-D float tensor of samples")


def _spectral_records(spectral, device, audio, ref_waves, aligned, frames, ref_frames) -> List[Dict]:
    """The spectral fields of every utterance: the waveforms against the recordings along the aligner's paths."""
    if spectral is None:
        from kokoro_ruslan_amd.spectral import SpectralDistance
        spectral = SpectralDistance(device=device)
    got = spectral.measure(audio, list(ref_waves), [al["path"] for al in aligned], frames, ref_frames)
    return [{k: g[k] for k in SPECTRAL_METRICS + SPECTRAL_COUNTS} for g in got]


def evaluate(engine, ids: Sequence[torch.Tensor], stress: Optional[Sequence[torch.Tensor]], ref_mels: Sequence[torch.Tensor], *,
             stream: bool = True, slots: int = 32, batch_size: int = 32, durations: Optional[Sequence[torch.Tensor]] = None,
             names: Optional[Sequence[str]] = None, mcep: int = 13, aligner=None, prosody=None, vocoder=None,
             vocoder_kwargs: Optional[Dict[str, Any]] = None, denoiser=None, denoise_strength: float = 0.005, extractor=None,
             ref_pitch: Optional[Sequence[torch.Tensor]] = None, ref_energy: Optional[Sequence[torch.Tensor]] = None,
             want_audio: bool = False, ref_waves: Optional[Sequence[torch.Tensor]] = None, spectral=None,
             phone_model: Optional[Dict] = None, phone_aligner=None, optional_ids=(),
             **controls) -> Union[Tuple[List[Dict], Dict[str, Any]], Tuple[List[Dict], Dict[str, Any], List[torch.Tensor]]]:
    """Synthesize every utterance free-running (generate_stream with `slots` rows, or generate_batch `batch_size` at a time) and
    compare it with ref_mels[i] [frames, n_mels].  controls: the stop controls of generate_batch.  Returns (records, summary):
    per utterance {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw" (dB), "mel_l1_dtw", "hit_bound" (the row ended at its
    generation bound, not by the stop rule)} and, with ground-truth `durations`, "dur_abs_err" = |sum predicted - sum true| frames;
    summarize() of them.  prosody: one kokoro_ruslan_amd.prosody.Prosody for every utterance or one per utterance (None: no controls):
    with the ground-truth durations forced, dur_abs_err is 0 and the other metrics are the decoder's alone.
    vocoder (a HifiganVocoder or GriffinLimVocoder; vocoder_kwargs go to its vocode()) adds the audio metrics: all mels are vocoded in
    one call, denoised by `denoiser` at denoise_strength if one is given (its bias set), their pitch and energy extracted by
    `extractor` (default: a FeatureExtractor on the engine's device) and compared with ref_pitch[i] / ref_energy[i] [ref frames] (the
    cache's normalised tracks; both required) along the mel's alignment.  Records gain "f0_rmse_cents", "f0_bias_cents", "gpe" (None
    when no step is voiced on both sides), "vuv_err", "energy_l1_dtw", the counts n_vv, n_vu, n_uv, n_uu, n_gpe
    (MelAligner.align(tracks=)) and "no_variance": an utterance whose reference pitch and energy are all zero comes from a cache
    written without them; it is marked and gets no track metrics.  want_audio=True returns (records, summary, waveforms).
    ref_waves (needs a vocoder): the recording of every utterance, 1-D float samples at 22050 Hz (of a corpus conditioned by
    kokoro-precompute --trim-silence / --loudness: its --conditioned-wavs).  The aligner is then asked for its paths and the (denoised)
    waveforms are measured against the recordings along them by `spectral` (default: a kokoro_ruslan_amd.spectral.SpectralDistance on
    the engine's device); every record gains sc_dtw_W, lsd_dtw_W, level_db_W for W in 256, 512, 1024, mr_sc_dtw, mr_lsd_dtw (None when
    a side is silent), spec_steps and spec_skipped.
    phone_model (a model of kokoro_ruslan_amd.align.PhoneAligner: kokoro-align --model-out; phone_aligner default: a PhoneAligner of
    the model's K and classes on the engine's device; optional_ids: the phoneme ids whose tokens may get no frame) asks what no warp
    can: whether the mel holds the phonemes that were requested.  The synthesized mels and ref_mels are each force-aligned to `ids`
    and scored in one PhoneAligner.score call; records gain "gop", "logpost", "phone_acc", "gop_min", "gop_min_token" (the synthesis),
    "ref_gop", "ref_logpost", "ref_phone_acc" (the recording) and "gop_gap", "phone_acc_gap" (synthesis - recording).  The phone model
    was fitted on recordings, so the recording's own score is the ceiling and the absolute numbers carry the model's fit: the gap is
    the number to read.  A side that cannot be aligned has None (so has the gap) and is counted in the summary's pron_infeasible.
    Without phone_model nothing of this is launched and the records are what they were."""
    N = len(ids)
    if len(ref_mels) != N:
        raise ValueError(f"{len(ref_mels)} reference mels for {N} utterances")
    for what, v in (("stress", stress), ("durations", durations), ("names", names)):
        if v is not None and len(v) != N:
            raise ValueError(f"{what}: {len(v)} entries for {N} utterances")
    _check_audio_args(N, vocoder, vocoder_kwargs, denoiser, denoise_strength, extractor, ref_pitch, ref_energy, want_audio, ref_waves,
                      spectral)
    if phone_model is None and (phone_aligner is not None or tuple(optional_ids)):
        raise ValueError("phone_aligner and optional_ids need a phone_model: they bear on the pronunciation scores alone")
    if N == 0:
        return ([], summarize([]), []) if want_audio else ([], summarize([]))
    if prosody is not None:
        from kokoro_ruslan_amd.prosody import as_list
        prosody = as_list(prosody, N)
    mels, info = _generate(engine, ids, stress, stream, slots, batch_size, controls, prosody)
    if aligner is None:
        from kokoro_ruslan_amd.dtw import MelAligner
        aligner = MelAligner(device=engine.device, K=mcep)
    audio, bare, spec = None, None, None
    if vocoder is None:
        aligned = aligner.align(mels, ref_mels)
    else:
        from kokoro.inference.audio import denoise, vocode
        from kokoro_ruslan_amd.dtw import MAX_FRAMES
        audio = vocode(vocoder, mels, **(vocoder_kwargs or {}))
        if denoiser is not None:
            audio = denoise(denoiser, audio, denoise_strength)
        if extractor is None:
            from kokoro_ruslan_amd.features import FeatureExtractor
            extractor = FeatureExtractor(device=engine.device)
        feats = extractor.extract(audio, max_seq_length=MAX_FRAMES + 1)      # (T or T + 1 frames of a T-frame mel: never cut short)
        tracks = {"pitch": ([f["pitch"] for f in feats], list(ref_pitch)), "energy": ([f["energy"] for f in feats], list(ref_energy))}
        if ref_waves is None:
            aligned = aligner.align(mels, ref_mels, tracks=tracks)
        else:
            aligned = aligner.align(mels, ref_mels, want_path=True, tracks=tracks)
            spec = _spectral_records(spectral, engine.device, audio, ref_waves, aligned, [int(m.shape[0]) for m in mels],
                                     [int(r.shape[0]) for r in ref_mels])
        where = torch.as_tensor(ref_pitch[0]).device                             # (one read for all utterances, wherever the tracks lie)
        bare = [n == 0 for n in torch.stack([(torch.count_nonzero(p) + torch.count_nonzero(e)).to(where)
                                             for p, e in zip(ref_pitch, ref_energy)]).tolist()]
    pron = None if phone_model is None else _pron_records(phone_aligner, phone_model, optional_ids, engine.device, mels, ref_mels, ids)
    records = []
    for i, (mel, al) in enumerate(zip(mels, aligned)):
        rec = {"name": names[i] if names is not None else i, "frames": int(mel.shape[0]), "ref_frames": int(ref_mels[i].shape[0]),
               "len_ratio": al["len_ratio"], "mcd_dtw": al["mcd_dtw"], "mel_l1_dtw": al["mel_l1_dtw"],
               "hit_bound": int(mel.shape[0]) >= int(info["bounds"][i][2])}
        if durations is not None:
            rec["dur_abs_err"] = abs(float(info["durations"][i].sum()) - float(durations[i].sum()))
        if bare is not None:
            rec["no_variance"] = bare[i]
            if not bare[i]:
                rec.update({k: al[k] for k in TRACK_METRICS + TRACK_COUNTS})
        if spec is not None:
            rec.update(spec[i])
        if pron is not None:
            rec.update(pron[i])
        records.append(rec)
    return (records, summarize(records), audio) if want_audio else (records, summarize(records))


def evaluate_vocoder(vocoder, ref_mels: Sequence[torch.Tensor], ref_waves: Sequence[torch.Tensor],
                     ref_pitch: Optional[Sequence[torch.Tensor]] = None, ref_energy: Optional[Sequence[torch.Tensor]] = None, *,
                     denoiser=None, denoise_strength: float = 0.005, vocoder_kwargs: Optional[Dict[str, Any]] = None, extractor=None,
                     aligner=None, spectral=None, names: Optional[Sequence[str]] = None, device="cuda", want_audio: bool = False):
    """Copy synthesis: the audio stage alone, with no acoustic model in the loop.  The cache's own mels ref_mels[i] [frames, n_mels] are
    vocoded (and denoised), aligned with themselves (the path is the diagonal) and the waveforms judged against the recordings
    ref_waves[i] like evaluate()'s: the fourth step of the error split none -> oracle durations -> oracle prosody -> copy synthesis.
    Returns (records, summary): per utterance {"name", "frames", the spectral fields} and, with ref_pitch and ref_energy (both or
    neither), "no_variance" and the track metrics of evaluate().  want_audio=True returns (records, summary, waveforms)."""
    N = len(ref_mels)
    if vocoder is None:
        raise ValueError("evaluate_vocoder needs a vocoder")
    if ref_waves is None:
        raise ValueError("evaluate_vocoder needs ref_waves: the recordings the audio is judged against")
    if (ref_pitch is None) != (ref_energy is None):
        raise ValueError("ref_pitch and ref_energy come together: both or neither")
    for what, v in (("ref_pitch", ref_pitch), ("ref_energy", ref_energy), ("names", names)):
        if v is not None and len(v) != N:
            raise ValueError(f"{what}: {len(v)} entries for {N} utterances")
    if vocoder_kwargs is not None and not isinstance(vocoder_kwargs, dict):
        raise ValueError("vocoder_kwargs must be a dict of keyword arguments for the vocoder's vocode()")
    if denoiser is not None and not (isinstance(denoise_strength, (int, float)) and math.isfinite(denoise_strength) and denoise_strength >= 0):
        raise ValueError(f"denoise_strength must be a finite number >= 0, not {denoise_strength!r}")
    _check_ref_waves(N, ref_waves, spectral)
    if N == 0:
        return ([], summarize([]), []) if want_audio else ([], summarize([]))
    from kokoro.inference.audio import denoise, vocode
    mels = list(ref_mels)
    audio = vocode(vocoder, mels, **(vocoder_kwargs or {}))
    if denoiser is not None:
        audio = denoise(denoiser, audio, denoise_strength)
    if aligner is None:
        from kokoro_ruslan_amd.dtw import MelAligner
        aligner = MelAligner(device=device)
    tracks, bare = None, None
    if ref_pitch is not None:
        from kokoro_ruslan_amd.dtw import MAX_FRAMES
        if extractor is None:
            from kokoro_ruslan_amd.features import FeatureExtractor
            extractor = FeatureExtractor(device=device)
        feats = extractor.extract(audio, max_seq_length=MAX_FRAMES + 1)
        tracks = {"pitch": ([f["pitch"] for f in feats], list(ref_pitch)), "energy": ([f["energy"] for f in feats], list(ref_energy))}
        where = torch.as_tensor(ref_pitch[0]).device
        bare = [n == 0 for n in torch.stack([(torch.count_nonzero(p) + torch.count_nonzero(e)).to(where)
                                             for p, e in zip(ref_pitch, ref_energy)]).tolist()]
    aligned = aligner.align(mels, mels, want_path=True, tracks=tracks)
    frames = [int(m.shape[0]) for m in mels]
    spec = _spectral_records(spectral, device, audio, ref_waves, aligned, frames, frames)
    records = []
    for i, al in enumerate(aligned):
        rec = {"name": names[i] if names is not None else i, "frames": frames[i]}
        if bare is not None:
            rec["no_variance"] = bare[i]
            if not bare[i]:
                rec.update({k: al[k] for k in TRACK_METRICS + TRACK_COUNTS})
        rec.update(spec[i])
        records.append(rec)
    summary = summarize(records)
    del summary["hit_bound_share"]                                            # (nothing was generated: no row has a bound)
    return (records, summary, audio) if want_audio else (records, summary)
