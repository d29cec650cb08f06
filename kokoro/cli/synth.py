"""`kokoro-synth`: mel spectrograms of many utterances from a kokoro-train checkpoint, decoded in batches on the engine.

    kokoro-synth --checkpoint CKPT (--features CACHE_DIR [--indices ...] | --ids FILE.jsonl) --output DIR
                 [--batch-size 32] [--weights auto|ema|model] [--stop-threshold X] [--max-len N] [--min-len-ratio R]
                 [--min-len-floor N] [--trim] [--math bf16|f32] [--stream [--slots 32]]
                 [--vocoder PATH [--vocoder-config JSON] [--vocoder-math bf16|f32] [--denoise [S]]]
                 [--griffin-lim [--griffin-lim-iters N] [--griffin-lim-seed S]]
                 [--loudness [LUFS] [--peak-db DB]]
                 [--speed F] [--pitch-scale F] [--pitch-shift F] [--energy-scale F] [--energy-shift F]
                 [--copy-prosody [durations|pitch|energy ...]]
                 [--documents [--gap-ms F] [--fade-ms F]] [--report FILE.json]

Writes <name>.npy per utterance: float32 [n_mels, frames], the vocoder's layout (reference inference/inference.py:623-631).
--features reads phoneme_indices / stress_indices from a precomputed feature cache (kokoro.data.cached); --ids reads JSON lines
{"name", "phoneme_indices", "stress_indices"?}.  --trim applies the reference's clamp + trailing-silence trim (:588-619).
--stream decodes all utterances in one pool of --slots rows whose finished rows are refilled with the next utterance (continuous
batching, KokoroEngine.generate_stream) instead of in fixed batches of --batch-size; the mels are the same.
--vocoder (a HiFi-GAN generator checkpoint: a directory with generator.pth + config.json, or a file) also writes <name>.wav: the
saved mel, clamped to [-11.5, 2] (:590), vocoded on the device in batches, int16 PCM at the vocoder config's sampling_rate.
--denoise (with --vocoder) takes the generator's stationary noise floor out of every waveform before it is written: S (default 0.005)
times the magnitude spectrum of what the generator makes of a silent mel is subtracted from the magnitude of every STFT frame, the
phase kept (kokoro_ruslan_amd.denoise).
--griffin-lim writes the same <name>.wav with the reference's Griffin-Lim vocoder instead (kokoro_ruslan_amd.griffinlim, 80 mels,
22050 Hz; :684-739), no checkpoint needed: N iterations (default 60) from random phases drawn under seed S (default: unseeded).
--loudness (with --vocoder or --griffin-lim) brings every waveform to LUFS (default -23) integrated loudness (ITU-R BS.1770-4,
kokoro_ruslan_amd.loudness) with its peak at or under --peak-db (default -1) dB of full scale, after --denoise and before the .wav is
written; the .wav then keeps that level instead of being peak-normalised.  A waveform shorter than one 400 ms block is left as it is.
--speed / --pitch-scale / --pitch-shift / --energy-scale / --energy-shift steer every utterance (kokoro_ruslan_amd.prosody.Prosody:
frames per phoneme divided by the speed, in [0.25, 4]; scale and shift on the normalised pitch of voiced frames and on the normalised
energy).  A line of --ids may carry "prosody": {...} with the fields of Prosody.from_json (also per-phoneme lists and forced
"durations" / "pitch" / "energy", and the frame-level "pitch_contour" / "energy_contour" / "contour_durations"); its fields override
the flags for that line.
--copy-prosody (with --features) synthesizes every cache utterance with its recording's prosody (Prosody.from_tracks): the cache
entry's phoneme durations forced and its frame-level pitch and energy put on every frame; named parts (durations, pitch, energy)
copy only those, e.g. `--copy-prosody pitch` carries the recording's intonation onto the model's own durations.  The other prosody
flags apply on top (--pitch-shift transposes the copied contour).  An utterance without durations in the cache, or asked for a track
the cache holds only zeros of (--no-variance), is an error that names it.
--documents (with --ids and --vocoder or --griffin-lim) is long-form synthesis, the last stretch of the reference's text_to_speech
(:566-648): a line of --ids may carry "document": "NAME"; the lines of one document are its chunks, played in file order, and a line
without the field is a document of its own named by its "name".  All chunks of all documents are synthesized in the one call, every mel
is health-checked, clamped and trimmed of its trailing silence on the device (kokoro_ruslan_amd.longform; <name>.npy is the finished
mel), vocoded (and denoised) per chunk, and the chunks of a document are joined with --gap-ms (default 150, the reference's 0.15 s) of
silence between them into <document>.wav; --loudness then works per document, so that a document has one level.  No per-chunk .wav is
written.  --fade-ms F (default 0: none, as the reference) fades every chunk in and out over F ms before the join.
--report FILE.json writes the health check per chunk: the mel's frames, kept frames, last voiced frame, threshold, min, max, mean, std,
NaN count and the flat flag (std < 1e-5, :579), its document and, with a vocoder, the waveform's peak before --loudness and the silent
flag (peak < 1e-4, :639).  The summary line names the chunks with NaNs, flat mels and silent audio."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import List, Optional, Tuple

import torch


def add_vocoder_flags(p: argparse.ArgumentParser) -> None:
    """The flags that name a vocoder (kokoro-synth and kokoro-eval spell them alike; check_vocoder_flags, load_vocoder)."""
    p.add_argument("--vocoder", metavar="PATH", default=None, help="HiFi-GAN generator: directory or checkpoint file")
    p.add_argument("--vocoder-config", metavar="JSON", default=None, help="HiFi-GAN config (default: the checkpoint's config.json)")
    p.add_argument("--vocoder-math", choices=("bf16", "f32"), default="bf16")
    p.add_argument("--denoise", type=float, nargs="?", const=0.005, default=None, metavar="S",
                   help="subtract S (default 0.005) times the vocoder's bias spectrum from every waveform (needs --vocoder)")
    p.add_argument("--griffin-lim", action="store_true", help="vocode with Griffin-Lim (no checkpoint; not with --vocoder)")
    p.add_argument("--griffin-lim-iters", type=int, default=60, metavar="N")
    p.add_argument("--griffin-lim-seed", type=int, default=None, metavar="S", help="seed of the initial random phases")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Batched mel synthesis from a Kokoro checkpoint (MI355X engine)")
    p.add_argument("--checkpoint", required=True)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", metavar="CACHE_DIR", help="precomputed feature cache (*.pt)")
    src.add_argument("--ids", metavar="FILE.jsonl", help='JSON lines {"name", "phoneme_indices", "stress_indices"?}')
    p.add_argument("--indices", type=int, nargs="*", default=None, help="utterances of the feature cache (its length-sorted order)")
    p.add_argument("--output", required=True)
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--weights", choices=("auto", "ema", "model"), default="auto")
    p.add_argument("--stop-threshold", type=float, default=None)
    p.add_argument("--max-len", type=int, default=None)
    p.add_argument("--min-len-ratio", type=float, default=None)
    p.add_argument("--min-len-floor", type=int, default=None)
    p.add_argument("--trim", action="store_true")
    p.add_argument("--math", choices=("bf16", "f32"), default="bf16")
    p.add_argument("--stream", action="store_true", help="continuous batching: refill finished rows instead of fixed batches")
    p.add_argument("--slots", type=int, default=None, metavar="N", help="rows of the --stream pool (default 32)")
    add_vocoder_flags(p)
    p.add_argument("--loudness", type=float, nargs="?", const=-23.0, default=None, metavar="LUFS",
                   help="bring every waveform to LUFS (default -23) integrated loudness (needs --vocoder or --griffin-lim)")
    p.add_argument("--peak-db", type=float, default=-1.0, metavar="DB", help="peak ceiling of --loudness in dB of full scale (default -1)")
    # (prosody flags leave no attribute behind when they are not given: an invocation without them parses as it always did)
    p.add_argument("--speed", type=float, default=argparse.SUPPRESS, metavar="F", help="frames per phoneme are divided by F, in [0.25, 4]")
    p.add_argument("--pitch-scale", type=float, default=argparse.SUPPRESS, metavar="F", help="factor on the normalised pitch of voiced frames (>= 0)")
    p.add_argument("--pitch-shift", type=float, default=argparse.SUPPRESS, metavar="F", help="added to the normalised pitch of voiced frames")
    p.add_argument("--energy-scale", type=float, default=argparse.SUPPRESS, metavar="F", help="factor on the normalised energy (>= 0)")
    p.add_argument("--energy-shift", type=float, default=argparse.SUPPRESS, metavar="F", help="added to the normalised energy")
    p.add_argument("--copy-prosody", nargs="*", choices=COPY_PARTS, default=argparse.SUPPRESS, metavar="PART",
                   help="with --features: force the recording's durations, pitch and energy (default all three) on every utterance")
    # (the long-form flags too leave no attribute behind when they are not given: long_form() reads them)
    p.add_argument("--documents", action="store_true", default=argparse.SUPPRESS,
                   help='long-form: join the chunks that share a "document" field of --ids into one <document>.wav')
    p.add_argument("--gap-ms", type=float, default=argparse.SUPPRESS, metavar="F", help="silence between the chunks of a document (default 150)")
    p.add_argument("--fade-ms", type=float, default=argparse.SUPPRESS, metavar="F", help="fade every chunk in and out over F ms (default 0: none)")
    p.add_argument("--report", metavar="FILE.json", default=argparse.SUPPRESS, help="write the per-chunk health check of mels and audio")
    return p


COPY_PARTS = ("durations", "pitch", "energy")


def check_vocoder_flags(p: argparse.ArgumentParser, args) -> None:
    if args.griffin_lim and args.vocoder:
        p.error("--griffin-lim and --vocoder are alternatives: give one")
    if not args.griffin_lim and (args.griffin_lim_iters != 60 or args.griffin_lim_seed is not None):
        p.error("--griffin-lim-iters / --griffin-lim-seed need --griffin-lim")
    if args.griffin_lim_iters < 0:
        p.error("--griffin-lim-iters must be >= 0")
    if args.denoise is not None:
        if args.griffin_lim or not args.vocoder:
            p.error("--denoise needs --vocoder: the bias it subtracts is a HiFi-GAN generator's (not with --griffin-lim)")
        if not math.isfinite(args.denoise) or args.denoise < 0:
            p.error("--denoise must be >= 0")


def check_args(p: argparse.ArgumentParser, args) -> None:
    check_vocoder_flags(p, args)
    if args.loudness is not None:
        if not (args.vocoder or args.griffin_lim):
            p.error("--loudness needs --vocoder or --griffin-lim: it works on the waveforms")
        if not math.isfinite(args.loudness):
            p.error("--loudness must be finite")
        if not math.isfinite(args.peak_db) or args.peak_db > 0:
            p.error("--peak-db must be <= 0")
    elif args.peak_db != -1.0:
        p.error("--peak-db needs --loudness")
    for flag in ("gap_ms", "fade_ms"):
        v = getattr(args, flag, 0.0)
        if not math.isfinite(v) or v < 0:
            p.error(f"--{flag.replace('_', '-')} must be >= 0")
    if getattr(args, "documents", False):
        if not args.ids:
            p.error('--documents needs --ids: the "document" field of its lines groups the chunks')
        if not (args.vocoder or args.griffin_lim):
            p.error("--documents needs --vocoder or --griffin-lim: it joins the waveforms")
    elif hasattr(args, "gap_ms") or hasattr(args, "fade_ms"):
        p.error("--gap-ms / --fade-ms need --documents")
    try:
        prosody_flags(args)
    except ValueError as e:
        p.error(str(e))
    if hasattr(args, "copy_prosody") and not args.features:
        p.error("--copy-prosody needs --features: the recorded prosody is the cache's")
    if args.slots is not None and not args.stream:
        p.error("--slots needs --stream")
    if args.slots is not None and args.slots < 1:
        p.error("--slots must be >= 1")


def read_ids(path: str) -> Tuple[List[str], List[torch.Tensor], Optional[List[torch.Tensor]]]:
    """(names, phoneme id vectors, stress vectors or None) of a JSON-lines file; stress is given on every line or on none."""
    names, ids, stress = [], [], []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            if "name" not in rec or "phoneme_indices" not in rec:
                raise ValueError(f"{path}:{n}: needs 'name' and 'phoneme_indices'")
            names.append(str(rec["name"]))
            ids.append(torch.tensor(rec["phoneme_indices"], dtype=torch.int64))
            st = rec.get("stress_indices")
            stress.append(torch.tensor(st, dtype=torch.int64) if st is not None else None)
            if st is not None and len(st) != len(rec["phoneme_indices"]):
                raise ValueError(f"{path}:{n}: stress_indices and phoneme_indices differ in length")
    if len(set(names)) != len(names):
        raise ValueError(f"{path}: duplicate names")
    if all(s is None for s in stress):
        return names, ids, None
    if any(s is None for s in stress):
        raise ValueError(f"{path}: stress_indices must be given on every line or on none")
    return names, ids, stress


PROSODY_FLAGS = ("speed", "pitch_scale", "pitch_shift", "energy_scale", "energy_shift")


def prosody_flags(args) -> dict:
    """The prosody flags given on the command line as Prosody.from_json fields (validated; ValueError names the flag's field)."""
    from kokoro_ruslan_amd.prosody import Prosody
    given = {k: getattr(args, k) for k in PROSODY_FLAGS if getattr(args, k, None) is not None}       # (absent unless given)
    Prosody.from_json(given, 1)
    return given


def read_prosody(path: str, flags: dict):
    """One Prosody per line of a --ids file: the line's "prosody" object over the flags (its fields win), or None when neither the
    flags nor any line asks for anything."""
    from kokoro_ruslan_amd.prosody import Prosody
    out, any_given = [], bool(flags)
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            own = rec.get("prosody")
            if own is not None and not isinstance(own, dict):
                raise ValueError(f"{path}:{n}: 'prosody' must be an object")
            any_given = any_given or own is not None
            try:
                out.append(Prosody.from_json({**flags, **(own or {})}, len(rec["phoneme_indices"])))
            except ValueError as e:
                raise ValueError(f"{path}:{n}: {e}") from None
    return out if any_given else None


def copy_parts(args) -> Tuple[str, ...]:
    """The parts --copy-prosody names (all three when it names none), () when the flag is not given."""
    if not hasattr(args, "copy_prosody"):
        return ()
    return tuple(k for k in COPY_PARTS if k in args.copy_prosody) or COPY_PARTS


def copied_prosody(names, ids, durs, pitch, energy, parts, flags: dict):
    """One Prosody per cache utterance that carries the recorded `parts` (Prosody.from_tracks) under the command line's flags;
    ValueError names an utterance whose cache entry lacks what is asked for."""
    from kokoro_ruslan_amd.prosody import Prosody
    out = []
    for name, u, dur, f0, en in zip(names, ids, durs, pitch, energy):
        if dur is None or dur.numel() != u.numel() or dur.numel() == 0 or bool((dur < 0).any()):
            raise ValueError(f"--copy-prosody: utterance {name} has no durations for its {int(u.numel())} phonemes in the cache")
        tracks = {}
        for part, t in (("pitch", f0), ("energy", en)):
            if part in parts:
                if not bool((t != 0).any()):
                    raise ValueError(f"--copy-prosody: utterance {name} has no {part} in the cache (written with --no-variance)")
                tracks[part] = t.float().reshape(-1).clamp(0.0, 1.0)
        try:
            out.append(Prosody.from_tracks(dur, tracks.get("pitch"), tracks.get("energy"), force_durations="durations" in parts,
                                           **flags).validate(int(u.numel())))
        except ValueError as e:
            raise ValueError(f"--copy-prosody: utterance {name}: {e}") from None
    return out


def long_form(args) -> Tuple[bool, float, float, Optional[str]]:
    """(--documents, --gap-ms, --fade-ms, --report) with their defaults where a flag was not given."""
    return getattr(args, "documents", False), getattr(args, "gap_ms", 150.0), getattr(args, "fade_ms", 0.0), getattr(args, "report", None)


def read_documents(path: str) -> Tuple[List[str], List[List[int]]]:
    """(document names in order of first appearance, the line numbers of every document's chunks in file order; lines counted as
    read_ids counts them) of a --ids file: a line's "document" field, or its "name" for a document of its own.  ValueError when a
    document's name is also that of another document or of a chunk of another document (their files would be confused)."""
    names, fields = [], []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            doc = rec.get("document")
            if doc is not None and (not isinstance(doc, str) or not doc):
                raise ValueError(f"{path}:{n}: 'document' must be a non-empty string, not {doc!r}")
            names.append(str(rec["name"]))
            fields.append(doc)
    explicit = {d for d in fields if d is not None}
    docs, members = [], {}
    for i, (name, doc) in enumerate(zip(names, fields)):
        if doc is None and name in explicit:
            raise ValueError(f"{path}: document {name!r} is named both by a line of its own and by a 'document' field")
        key = name if doc is None else doc
        if key not in members:
            docs.append(key)
            members[key] = []
        members[key].append(i)
    for i, (name, doc) in enumerate(zip(names, fields)):
        if name in members and i not in members[name]:
            raise ValueError(f"{path}: {name!r} names a document and a chunk of document {doc!r}")
    return docs, [members[d] for d in docs]


def read_features(cache_dir: str, indices=None, tracks: bool = False):
    """(names, ids, stress) of the cache's utterances; with tracks also (durations, pitch [T], energy [T]) of every one."""
    from kokoro.data.cached import CachedFeatureDataset
    ds = CachedFeatureDataset(cache_dir, indices=indices, memory_cache=False)
    names, ids, stress, durs, pitch, energy = [], [], [], [], [], []
    for i in range(len(ds)):
        it = ds[i]
        names.append(os.path.splitext(ds.samples[i]["file"].name)[0])
        ids.append(it["phoneme_indices"].to(torch.int64))
        stress.append(it["stress_indices"].to(torch.int64))
        if tracks:
            durs.append(it["phoneme_durations"].to(torch.int64))
            pitch.append(it["pitch"].float().reshape(-1))
            energy.append(it["energy"].float().reshape(-1))
    return (names, ids, stress, durs, pitch, energy) if tracks else (names, ids, stress)


def level_and_write(args, names, audio, sample_rate: int, device) -> str:
    """Write <name>.wav per waveform; with --loudness at that level (not peak-normalised).  Returns what to add to the summary line."""
    from kokoro.inference.audio import normalise_loudness, write_wav
    note = ""
    if args.loudness is not None:
        from kokoro_ruslan_amd.loudness import LoudnessNormaliser
        peak_db = args.peak_db
        audio, info = normalise_loudness(LoudnessNormaliser(device=device, sample_rate=sample_rate), audio, args.loudness, peak_db)
        limited = [n for n, i in zip(names, info) if i["limited"]]
        unmeasured = [n for n, i in zip(names, info) if i["measured"] is None]
        note = f", {args.loudness:g} LUFS under {peak_db:g} dB"
        if limited:
            note += f", {len(limited)} peak-limited: {' '.join(limited)}"
        if unmeasured:
            note += f", {len(unmeasured)} too short or quiet to measure: {' '.join(unmeasured)}"
    for name, a in zip(names, audio):
        write_wav(os.path.join(args.output, f"{name}.wav"), a, sample_rate, normalise=args.loudness is None)
    return note


SILENT_PEAK = 1e-4        # the reference's near-silence warning (inference.py:639)


def health_note(names, info) -> str:
    """What the mel health check (inference.py:569-580) adds to the summary line: the chunks with NaNs and the flat ones, by name."""
    if info is None:
        return ""
    note = ""
    for what, bad in (("with NaNs", [n for n, i in zip(names, info) if i["nan"]]), ("flat", [n for n, i in zip(names, info) if i["flat"]])):
        if bad:
            note += f", {len(bad)} {what}: {' '.join(bad)}"
    return note


def check_vocoder_model(p: argparse.ArgumentParser, args, n_mels: int) -> None:
    """What the vocoder the flags name asks of the checkpoint, once it is loaded."""
    if args.griffin_lim and n_mels != 80:
        p.error(f"--griffin-lim needs an 80-mel model; this checkpoint makes {n_mels} mel channels")


def load_vocoder(args, device):
    """(vocoder, the keyword arguments of its vocode(), denoiser or None, what they do) for the vocoder the flags name: a HiFi-GAN
    generator (with --denoise: a SpectralDenoiser holding its bias) or Griffin-Lim with its iterations and seeded phases."""
    if args.vocoder:
        from kokoro_ruslan_amd.vocoder import HifiganVocoder
        voc = HifiganVocoder.from_checkpoint(args.vocoder, args.vocoder_config, device=device, math_mode=args.vocoder_math)
        den, how = None, f"{args.vocoder_math} vocoder"
        if args.denoise is not None:
            from kokoro_ruslan_amd.denoise import SpectralDenoiser
            den = SpectralDenoiser(device=device)
            den.bias_from_vocoder(voc)
            how += f", denoised at strength {args.denoise:g}"
        return voc, {}, den, how
    from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
    gen = torch.Generator().manual_seed(args.griffin_lim_seed) if args.griffin_lim_seed is not None else None
    return (GriffinLimVocoder(device=device), dict(n_iter=args.griffin_lim_iters, generator=gen), None,
            f"Griffin-Lim, {args.griffin_lim_iters} iterations")


def vocode_all(args, engine, mels):
    """(waveforms of the mels in input order, sample rate, what was done) with the vocoder the flags name, denoised with --denoise."""
    from kokoro.inference.audio import denoise, vocode
    voc, kwargs, den, how = load_vocoder(args, engine.device)
    audio = vocode(voc, mels, **kwargs)
    if den is not None:
        audio = denoise(den, audio, args.denoise)
    return audio, voc.sampling_rate, how


def main(argv=None) -> int:
    import numpy as np
    from kokoro.inference.synth import load_for_inference, synthesize, trim_trailing_silence
    parser = build_parser()
    args = parser.parse_args(argv)
    check_args(parser, args)
    flags = prosody_flags(args)
    by_document, gap_ms, fade_ms, report = long_form(args)
    if args.ids:
        names, ids, stress = read_ids(args.ids)
        prosody = read_prosody(args.ids, flags)
    else:
        parts = copy_parts(args)
        if parts:
            names, ids, stress, durs, pitch, energy = read_features(args.features, args.indices, tracks=True)
            try:
                prosody = copied_prosody(names, ids, durs, pitch, energy, parts, flags)
            except ValueError as e:
                parser.error(str(e))
        else:
            names, ids, stress = read_features(args.features, args.indices)
            prosody = None
        if flags and not parts:
            from kokoro_ruslan_amd.prosody import Prosody
            prosody = Prosody.from_json(flags, 1)              # (scalars only: one entry serves every utterance)
    engine, controls, used = load_for_inference(args.checkpoint, weights=args.weights, math_mode=args.math, max_len=args.max_len,
                                                stop_threshold=args.stop_threshold, min_len_ratio=args.min_len_ratio,
                                                min_len_floor=args.min_len_floor)
    check_vocoder_model(parser, args, engine.dims.mel)
    pkw = {} if prosody is None else {"prosody": prosody}
    if args.stream:
        mels = synthesize(engine, ids, stress, stream=True, slots=32 if args.slots is None else args.slots, **pkw, **controls.kwargs())
    else:
        mels = synthesize(engine, ids, stress, batch_size=args.batch_size, **pkw, **controls.kwargs())
    os.makedirs(args.output, exist_ok=True)
    finished, info = None, None
    if by_document:
        doc_names, documents = read_documents(args.ids)
    if by_document or report:
        from kokoro.inference.audio import finish_mels
        from kokoro_ruslan_amd.longform import MelFinisher
        finished, info = finish_mels(MelFinisher(device=engine.device, n_mels=engine.dims.mel), mels)
    saved = []
    for i, (name, mel) in enumerate(zip(names, mels)):
        mel = finished[i].cpu() if by_document else mel.float().cpu()
        if args.trim and not by_document:                   # (a finished mel is trimmed already)
            mel = trim_trailing_silence(mel)
        np.save(os.path.join(args.output, f"{name}.npy"), mel.t().contiguous().numpy().astype(np.float32))
        saved.append(mel)
    print(f"kokoro-synth: {len(mels)} mels ({used} weights, {controls}{health_note(names, info)}) -> {args.output}")
    peaks = None
    if args.vocoder or args.griffin_lim:
        audio, rate, how = vocode_all(args, engine, finished if by_document else saved)
        if info is not None:
            from kokoro.inference.audio import join_chunks
            joined, peaks = join_chunks(audio, documents if by_document else [[i] for i in range(len(audio))], rate,
                                        gap_ms, fade_ms)
            peaks = peaks.cpu().tolist()
            silent = [n for n, pk in zip(names, peaks) if pk < SILENT_PEAK]
            if silent:
                how += f", {len(silent)} nearly silent: {' '.join(silent)}"
        if by_document:
            how += f", {gap_ms:g} ms gaps" + (f", {fade_ms:g} ms fades" if fade_ms else "")
            how += level_and_write(args, doc_names, joined, rate, engine.device)
            print(f"kokoro-synth: {len(audio)} chunks in {len(doc_names)} documents at {rate} Hz ({how}) -> {args.output}")
        else:
            how += level_and_write(args, names, audio, rate, engine.device)
            print(f"kokoro-synth: {len(audio)} waveforms at {rate} Hz ({how}) -> {args.output}")
    if report:
        of = {c: d for d, members in zip(doc_names, documents) for c in members} if by_document else {}
        entries = []
        for i, (name, rec) in enumerate(zip(names, info)):
            entry = {"name": name, "document": of.get(i, name), **rec}
            if peaks is not None:
                entry.update(audio_peak=peaks[i], silent=bool(peaks[i] < SILENT_PEAK))
            entries.append(entry)
        with open(report, "w") as f:
            json.dump(entries, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
