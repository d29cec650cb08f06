"""kokoro-precompute: write the feature cache kokoro-train reads, with the acoustic features extracted on the device.

    kokoro-precompute --wavs DIR --ids FILE.jsonl --cache-dir OUT [--force] [--no-variance] [--resample] [--batch-size N]
                      [--max-seq-length N] [--trim-silence [DB]] [--loudness [LUFS]] [--peak-db DB] [--conditioned-wavs DIR]

FILE.jsonl is kokoro-synth --ids's format, one utterance per line: {"name", "phoneme_indices"[, "stress_indices"]}, plus optional
"phoneme_durations" (frames per phoneme, from kokoro-align or an MFA alignment; absent: the reference's even fallback estimate) and "text".
DIR/<name>.wav is the audio, 22050 Hz; with --resample audio at another rate is resampled to 22050 Hz on the device first (the
reference's torchaudio.transforms.Resample, data/dataset.py:662-665) instead of being refused.  The phonemizer and MFA alignment are
not part of this tool: it takes their results.  Entries of the current cache version are skipped unless --force, as the reference's kokoro-precompute does.
--trim-silence cuts what lies more than DB (default 40) dB under the loudest frame at either end of every waveform, keeping 50 ms
(the reference trims its corpus with a VAD before alignment, cli/preprocess.py:24-33); --loudness scales every waveform to LUFS
(default -23) integrated loudness under a peak of --peak-db (default -1) dB (kokoro_ruslan_amd.loudness).  Both run on the device
after --resample and before the features, which are computed from the conditioned fp32 audio.  Durations made for the untrimmed audio
no longer fit: --trim-silence refuses an --ids file that carries phoneme_durations; run kokoro-align on the new cache afterwards.
--conditioned-wavs DIR writes every conditioned waveform as DIR/<name>.wav (int16: the rounding of the audio the features saw), so a
corpus that trains with speed perturbation can point {data_dir}/wavs at audio that matches the cache.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import Dict, List


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="kokoro-precompute", description=__doc__.split("\n\n")[0])
    p.add_argument("--wavs", required=True, metavar="DIR")
    p.add_argument("--ids", required=True, metavar="FILE.jsonl")
    p.add_argument("--cache-dir", required=True, metavar="OUT")
    p.add_argument("--force", action="store_true", help="recompute entries that exist")
    p.add_argument("--no-variance", action="store_true", help="zero pitch and energy")
    p.add_argument("--resample", action="store_true", help="resample audio at another rate to 22050 Hz on the device instead of refusing it")
    p.add_argument("--batch-size", type=int, default=32, help="utterances per device call")
    p.add_argument("--max-seq-length", type=int, default=1800, help="mel frames kept per utterance")
    p.add_argument("--trim-silence", type=float, nargs="?", const=40.0, default=None, metavar="DB",
                   help="cut leading and trailing audio more than DB (default 40) dB under the loudest frame, keeping 50 ms; not with "
                        "phoneme_durations in --ids: run kokoro-align afterwards")
    p.add_argument("--loudness", type=float, nargs="?", const=-23.0, default=None, metavar="LUFS",
                   help="scale every waveform to LUFS (default -23) integrated loudness")
    p.add_argument("--peak-db", type=float, default=-1.0, metavar="DB", help="peak ceiling of --loudness in dB of full scale (default -1)")
    p.add_argument("--conditioned-wavs", metavar="DIR", default=None,
                   help="write every trimmed / levelled waveform as DIR/<name>.wav (needs --trim-silence or --loudness)")
    p.add_argument("--n-mels", type=int, default=80)
    p.add_argument("--hop-length", type=int, default=256)
    p.add_argument("--sample-rate", type=int, default=22050)
    return p


def check_args(p: argparse.ArgumentParser, args) -> None:
    for flag, got, want in (("--n-mels", args.n_mels, 80), ("--hop-length", args.hop_length, 256), ("--sample-rate", args.sample_rate, 22050)):
        if got != want:
            p.error(f"{flag} {got}: the feature kernels are built for {want} (the reference's default)")
    if args.batch_size < 1:
        p.error("--batch-size must be >= 1")
    if args.max_seq_length < 1:
        p.error("--max-seq-length must be >= 1")
    if args.trim_silence is not None and not (math.isfinite(args.trim_silence) and args.trim_silence > 0):
        p.error("--trim-silence must be > 0 (dB under the loudest frame)")
    if args.loudness is not None:
        if not math.isfinite(args.loudness):
            p.error("--loudness must be finite")
        if not math.isfinite(args.peak_db) or args.peak_db > 0:
            p.error("--peak-db must be <= 0")
    elif args.peak_db != -1.0:
        p.error("--peak-db needs --loudness")
    if args.conditioned_wavs is not None and args.trim_silence is None and args.loudness is None:
        p.error("--conditioned-wavs needs --trim-silence or --loudness: there is nothing else to write")


def read_extras(path: str) -> Dict[str, Dict]:
    """name -> {"phoneme_durations": list | None, "text": str} of the JSON-lines file (read_ids has validated the rest)."""
    extras = {}
    with open(path) as f:
        for line in f:
            if line.strip():
                rec = json.loads(line)
                extras[str(rec["name"])] = {"phoneme_durations": rec.get("phoneme_durations"), "text": str(rec.get("text", ""))}
    return extras


def main(argv=None) -> int:
    p = build_parser()
    args = p.parse_args(argv)
    check_args(p, args)
    import torch
    from kokoro.cli.synth import read_ids
    from kokoro.data import features as DF
    from kokoro_ruslan_amd.features import FeatureExtractor

    names, ids, stress = read_ids(args.ids)
    extras = read_extras(args.ids)
    if args.trim_silence is not None:
        for name in names:
            if extras[name]["phoneme_durations"] is not None:
                p.error(f"--trim-silence: {name} carries phoneme_durations, which were made for the untrimmed audio and no longer sum "
                        f"to the trimmed length; drop them from {args.ids} and run kokoro-align on the new cache")
    conditioning = args.trim_silence is not None or args.loudness is not None
    norm = None
    trimmed_samples = limited = unmeasured = 0
    if args.conditioned_wavs is not None:
        os.makedirs(args.conditioned_wavs, exist_ok=True)
    todo: List[int] = []
    skipped = 0
    for i, name in enumerate(names):
        if not args.force and DF.is_current(DF.cache_path(args.cache_dir, name)):
            skipped += 1
        else:
            todo.append(i)
    computed = failed = 0
    ext = FeatureExtractor() if todo else None
    rs = None
    for s in range(0, len(todo), args.batch_size):
        batch, waves, rates = [], [], []
        for i in todo[s:s + args.batch_size]:
            try:
                path = os.path.join(args.wavs, names[i] + ".wav")
                sr, w = DF.load_wav_any(path) if args.resample else (args.sample_rate, DF.load_wav(path))
                waves.append(w)
                rates.append(sr)
                batch.append(i)
            except Exception as e:
                failed += 1
                print(f"kokoro-precompute: {names[i]}: {e}", file=sys.stderr)
        if not batch:
            continue
        if any(sr != args.sample_rate for sr in rates):
            try:
                if rs is None:
                    from kokoro_ruslan_amd.resample import Resampler
                    rs = Resampler()
                waves = rs.resample(waves, rates, args.sample_rate)
            except Exception as e:
                failed += len(batch)
                print(f"kokoro-precompute: resampling the batch of {names[batch[0]]}: {e}", file=sys.stderr)
                continue
        if conditioning:
            try:
                if norm is None:
                    from kokoro_ruslan_amd.loudness import LoudnessNormaliser
                    norm = LoudnessNormaliser(sample_rate=args.sample_rate)
                before = [int(w.numel()) for w in waves]
                if args.loudness is not None:
                    waves, info = norm.normalise(waves, args.loudness, args.peak_db, trim_db=args.trim_silence)
                    limited += sum(i["limited"] for i in info)
                    unmeasured += sum(i["measured"] is None for i in info)
                else:
                    waves = [w[s0:e0] for w, (s0, e0) in zip(waves, norm.trim_edges(waves, args.trim_silence))]
                trimmed_samples += sum(before) - sum(int(w.numel()) for w in waves)
                if args.conditioned_wavs is not None:
                    from kokoro.inference.audio import write_wav
                    for i, w in zip(batch, waves):
                        write_wav(os.path.join(args.conditioned_wavs, names[i] + ".wav"), w, args.sample_rate, normalise=False)
            except Exception as e:
                failed += len(batch)
                print(f"kokoro-precompute: conditioning the batch of {names[batch[0]]}: {e}", file=sys.stderr)
                continue
        feats = ext.extract(waves, max_seq_length=args.max_seq_length, variance=not args.no_variance)
        for i, ft in zip(batch, feats):
            try:
                x = extras[names[i]]
                dur = torch.tensor(x["phoneme_durations"], dtype=torch.long) if x["phoneme_durations"] is not None else None
                entry = DF.cache_entry(ft, names[i], ids[i], stress[i] if stress is not None else None, dur, x["text"])
                DF.write_cache_entry(args.cache_dir, entry)
                computed += 1
            except Exception as e:
                failed += 1
                print(f"kokoro-precompute: {names[i]}: {e}", file=sys.stderr)
    if conditioning:
        what = [f"{trimmed_samples} samples trimmed"] if args.trim_silence is not None else []
        if args.loudness is not None:
            what.append(f"{limited} gains peak-limited, {unmeasured} waveforms too short or quiet to measure (left at gain 1)")
        print(f"kokoro-precompute: conditioning: {', '.join(what)}")
    print(f"kokoro-precompute: {computed} computed, {skipped} skipped, {failed} failed ({len(names)} utterances) -> {args.cache_dir}")
    return 0 if failed == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
