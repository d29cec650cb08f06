"""`kokoro-eval`: free-running evaluation of a kokoro-train checkpoint against the ground-truth mels of a feature cache.

    kokoro-eval --checkpoint CKPT --features CACHE_DIR [--indices ...] [--split val|train|all] [--validation-split 0.1]
                [--weights auto|ema|model] [--math bf16|f32] [--no-stream] [--slots N] [--batch-size N] [--mcep K]
                [--stop-threshold X] [--max-len N] [--min-len-ratio R] [--min-len-floor N] [--output REPORT.json]
                [--oracle-durations] [--oracle-prosody]
                [--vocoder PATH [--vocoder-config JSON] [--vocoder-math bf16|f32] [--denoise [S]]]
                [--griffin-lim [--griffin-lim-iters N] [--griffin-lim-seed S]] [--gpe-ratio F]
                [--wavs DIR [--copy-synthesis]]
                [--pronunciation [MODEL] [--align-iters N] [--align-states S] [--align-mixtures M] [--optional-id ID ...] [--pronunciation-tokens]]

Synthesizes every selected utterance with the stop rule deciding its length (continuous batching in a pool of --slots rows, or with
--no-stream in batches of --batch-size), aligns each mel with the cached ground truth by dynamic time warping on K mel cepstra and
prints, one line per metric, the mean, median and 95th percentile of: mcd_dtw (mel-cepstral distortion along the path, dB),
mel_l1_dtw (mean |difference| of the aligned log-mels), len_ratio (synthesized / true frames), dur_abs_err (|sum of predicted
durations - sum of true ones|, frames); plus the share of utterances that ran into their generation bound.  --split val takes the
utterances `kokoro-train --validation-split` holds out (the same draw: kokoro.data.cached.split_indices), --indices names utterances
of the cache's length-sorted order instead.  --output writes records, summary, controls and the weights used as JSON.
--oracle-durations forces the cache's phoneme_durations on every utterance (kokoro_ruslan_amd.prosody): dur_abs_err is then 0 and
len_ratio, mcd_dtw and mel_l1_dtw are free of the duration predictor's errors; the pitch and energy predictors still run.  An
utterance whose cache entry holds no durations for its phonemes is an error that names it.
--oracle-prosody (implies --oracle-durations) also forces the cache entry's frame-level pitch and energy on every frame
(Prosody.from_tracks: the condition the decoder was trained on), so that the three numbers show the decoder alone; the differences
none -> --oracle-durations -> --oracle-prosody split the error into the duration predictor's share, the pitch and energy predictors'
share and the decoder's.  An utterance without durations, or whose cached pitch and energy are all zero (a --no-variance cache), is an
error that names it.
--vocoder / --griffin-lim (kokoro-synth's flags and loaders; --denoise with --vocoder) judge the audio too: every mel is vocoded, the
pitch and energy of the waveforms are extracted on the device (kokoro_ruslan_amd.features) and compared with the cache entry's own
pitch and energy along the same alignment.  The report then also carries f0_rmse_cents and f0_bias_cents (root mean square and mean
of 1200 log2(f_syn / f_true) over the steps voiced on both sides), gpe (the share of those steps whose F0 is more than --gpe-ratio,
default 0.2, off the true one), vuv_err (the share of steps voiced on one side only) and energy_l1_dtw (mean |difference| of the
normalised energies).  An utterance whose cached pitch and energy are all zero (a cache written with --no-variance) gets none of them
and is counted in the summary line.
--wavs DIR (with --vocoder or --griffin-lim) names the speaker's recordings, DIR/<name>.wav as kokoro-precompute --wavs finds them
(22050 Hz mono; a missing file or another rate is named and the exit status is 1).  Every waveform is then also held against its
recording along the same alignment (kokoro_ruslan_amd.spectral): sc_dtw_W (spectral convergence at the least-squares gain),
level_db_W (how much louder the synthesized spectrum sits, dB) and lsd_dtw_W (log-spectral distance with that offset taken out, dB) at
analysis windows W = 256, 512, 1024, and their means mr_sc_dtw and mr_lsd_dtw: the numbers that move with the vocoder, --denoise and
--griffin-lim-iters.  A corpus conditioned with kokoro-precompute --trim-silence / --loudness must be compared against its
--conditioned-wavs directory, not the raw recordings: the cache's frames count the conditioned audio.
--copy-synthesis (needs --wavs and a vocoder; --checkpoint is optional with it and ignored) leaves the acoustic model out: the cache's
own mels are vocoded and judged against the recordings, the audio stage's share of the error and the last step of the split.
--pronunciation [MODEL] asks what no warp can: whether the mel holds the phonemes that were requested.  The synthesized mels and the
cache's own are force-aligned to the phoneme ids with a phone model (kokoro_ruslan_amd.align.PhoneAligner.score) -- the file saved by
kokoro-align --model-out (another K or class count is named and the exit status is 1), or, without a file, one fitted on the selection's
cached mels (--align-iters N passes, default 6); --optional-id names phoneme ids whose tokens may get no frame.  The report gains gop
(mean over the frames of log-likelihood(forced phoneme) - log-likelihood(best phoneme)), logpost (mean log posterior of the forced
phoneme), phone_acc (share of frames whose best phoneme is the forced one), gop_min / gop_min_token (the worst token), ref_gop,
ref_logpost, ref_phone_acc (the recording) and gop_gap, phone_acc_gap (synthesis - recording); an utterance a side of which cannot be
aligned has null there and is counted.  The model was fitted on recordings, so the recording's score is the ceiling: read the gap.
--pronunciation-tokens adds the per-token lists (pron_tokens, ref_pron_tokens) to the records of --output.  A MODEL of 2 or 3 states
per phoneme (kokoro-align --states) is taken as it is; --align-states S gives the model fitted here that many (default 1).  A frame's
phoneme likelihood is then that of the phoneme's best state.  A MODEL of 2 or 4 Gaussians per state (kokoro-align --mixtures) is taken as
it is too; --align-mixtures M gives the model fitted here that many (default 1)."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import List, Optional

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Free-running evaluation of a Kokoro checkpoint: MCD-DTW against a feature cache")
    p.add_argument("--checkpoint", required=True)      # (parse(): optional with --copy-synthesis, and only with it)
    p.add_argument("--features", metavar="CACHE_DIR", required=True, help="precomputed feature cache (*.pt)")
    p.add_argument("--indices", type=int, nargs="*", default=None, help="utterances of the feature cache (its length-sorted order)")
    p.add_argument("--split", choices=("val", "train", "all"), default=None, help="default: val (all with --indices)")
    p.add_argument("--validation-split", type=float, default=0.1)
    p.add_argument("--weights", choices=("auto", "ema", "model"), default="auto")
    p.add_argument("--math", choices=("bf16", "f32"), default="bf16")
    p.add_argument("--no-stream", action="store_true", help="fixed batches of --batch-size instead of continuous batching")
    p.add_argument("--slots", type=int, default=None, metavar="N", help="rows of the continuous-batching pool (default 32)")
    p.add_argument("--batch-size", type=int, default=None, metavar="N", help="with --no-stream (default 32)")
    p.add_argument("--mcep", type=int, default=13, metavar="K", help="cepstral coefficients c1..cK of the distance (default 13)")
    p.add_argument("--stop-threshold", type=float, default=None)
    p.add_argument("--max-len", type=int, default=None)
    p.add_argument("--min-len-ratio", type=float, default=None)
    p.add_argument("--min-len-floor", type=int, default=None)
    p.add_argument("--output", metavar="REPORT.json", default=None)
    p.add_argument("--oracle-durations", action="store_true", help="synthesize on the cache's phoneme_durations instead of the predicted ones")
    # (leaves no attribute behind when it is not given: an invocation without it parses as it always did)
    p.add_argument("--oracle-prosody", action="store_true", default=argparse.SUPPRESS,
                   help="also force the cache's frame-level pitch and energy (implies --oracle-durations)")
    from kokoro.cli.synth import add_vocoder_flags
    add_vocoder_flags(p)
    p.add_argument("--gpe-ratio", type=float, default=0.2, metavar="F",
                   help="a gross pitch error: F0 more than F times the true one off it (default 0.2; needs --vocoder or --griffin-lim)")
    # (like --oracle-prosody these leave no attribute behind when they are not given)
    p.add_argument("--wavs", metavar="DIR", default=argparse.SUPPRESS,
                   help="the recordings, DIR/<name>.wav at 22050 Hz: adds the spectral distance of the vocoded audio to them (needs "
                        "--vocoder or --griffin-lim).  For a cache made with kokoro-precompute --trim-silence / --loudness give its "
                        "--conditioned-wavs directory")
    p.add_argument("--copy-synthesis", action="store_true", default=argparse.SUPPRESS,
                   help="vocode the cache's own mels instead of synthesized ones: the vocoder and denoiser alone (needs --wavs and a "
                        "vocoder; --checkpoint is optional)")
    p.add_argument("--pronunciation", nargs="?", const="", default=argparse.SUPPRESS, metavar="MODEL",
                   help="score every mel against its phonemes with a phone model: MODEL saved by kokoro-align --model-out, or, without "
                        "a file, one fitted on the cached mels of the selection")
    p.add_argument("--align-iters", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="passes of Viterbi training when --pronunciation fits its model (default 6)")
    p.add_argument("--align-states", type=int, default=argparse.SUPPRESS, metavar="S",
                   help="states per phoneme (1..3, default 1) of the model --pronunciation fits")
    p.add_argument("--align-mixtures", type=int, default=argparse.SUPPRESS, metavar="M",
                   help="Gaussians per state (1, 2 or 4, default 1) of the model --pronunciation fits")
    p.add_argument("--optional-id", type=int, action="append", default=argparse.SUPPRESS, metavar="ID",
                   help="a phoneme id whose tokens may get no frame (with --pronunciation; may be repeated)")
    p.add_argument("--pronunciation-tokens", action="store_true", default=argparse.SUPPRESS,
                   help="add the per-token scores to the records of --output (with --pronunciation)")
    return p


def parse(argv=None):
    """(parser, args): --checkpoint is required unless --copy-synthesis is given."""
    p = build_parser()
    if "--copy-synthesis" in (sys.argv[1:] if argv is None else list(argv)):
        for a in p._actions:
            if a.dest == "checkpoint":
                a.required, a.default = False, None
    return p, p.parse_args(argv)


def check_args(p: argparse.ArgumentParser, args) -> None:
    if args.indices is not None and args.split is not None:
        p.error("--indices and --split are alternatives: give one")
    if args.indices is not None and (not args.indices or min(args.indices) < 0):
        p.error("--indices needs non-negative utterance numbers")
    if not (0.0 < args.validation_split < 1.0):
        p.error("--validation-split must be in (0, 1)")
    if args.slots is not None and args.no_stream:
        p.error("--slots is for the continuous-batching pool: not with --no-stream")
    if args.batch_size is not None and not args.no_stream:
        p.error("--batch-size needs --no-stream")
    if args.slots is not None and args.slots < 1:
        p.error("--slots must be >= 1")
    if args.batch_size is not None and args.batch_size < 1:
        p.error("--batch-size must be >= 1")
    if not (1 <= args.mcep <= 32):
        p.error("--mcep must be in 1..32")
    from kokoro.cli.synth import check_vocoder_flags
    check_vocoder_flags(p, args)
    if args.gpe_ratio != 0.2 and not (args.vocoder or args.griffin_lim):
        p.error("--gpe-ratio needs --vocoder or --griffin-lim: it bears on the audio's F0")
    if not math.isfinite(args.gpe_ratio) or args.gpe_ratio < 0:
        p.error("--gpe-ratio must be >= 0")
    if getattr(args, "oracle_prosody", False):
        args.oracle_durations = True
    if hasattr(args, "wavs") and not (args.vocoder or args.griffin_lim):
        p.error("--wavs needs --vocoder or --griffin-lim: the recordings are compared with the vocoded audio")
    if getattr(args, "copy_synthesis", False):
        if not hasattr(args, "wavs"):
            p.error("--copy-synthesis needs --wavs: the vocoded mels are judged against the recordings")
        if args.oracle_durations:
            p.error("--copy-synthesis synthesizes nothing: not with --oracle-durations / --oracle-prosody")
    elif args.checkpoint is None:
        p.error("the following arguments are required: --checkpoint")
    if not hasattr(args, "pronunciation"):
        for flag in ("align_iters", "align_states", "align_mixtures", "optional_id", "pronunciation_tokens"):
            if hasattr(args, flag):
                p.error(f"--{flag.replace('_', '-')} needs --pronunciation")
        return
    if getattr(args, "copy_synthesis", False):
        p.error("--pronunciation scores synthesized mels: not with --copy-synthesis")
    if hasattr(args, "align_iters") and args.pronunciation:
        p.error("--align-iters is for fitting a model: not with --pronunciation MODEL")
    if getattr(args, "align_iters", 6) < 1:
        p.error("--align-iters must be >= 1")
    if hasattr(args, "align_states") and args.pronunciation:
        p.error("--align-states is for fitting a model: not with --pronunciation MODEL (the file's states hold)")
    if not (1 <= getattr(args, "align_states", 1) <= 3):
        p.error("--align-states must be 1, 2 or 3")
    if hasattr(args, "align_mixtures") and args.pronunciation:
        p.error("--align-mixtures is for fitting a model: not with --pronunciation MODEL (the file's mixtures hold)")
    if getattr(args, "align_mixtures", 1) not in (1, 2, 4):
        p.error("--align-mixtures must be 1, 2 or 4")
    if any(o < 0 for o in getattr(args, "optional_id", [])):
        p.error("--optional-id must be a phoneme id >= 0")


def read_wavs(wav_dir: str, names: List[str]) -> List[torch.Tensor]:
    """DIR/<name>.wav of every utterance, mono fp32 at 22050 Hz; ValueError names a missing file or another rate."""
    from kokoro.data.features import load_wav
    out = []
    for name in names:
        path = os.path.join(wav_dir, name + ".wav")
        if not os.path.isfile(path):
            raise ValueError(f"{path}: no such recording (--wavs expects <name>.wav for every utterance of the selection)")
        out.append(load_wav(path))
    return out


def _print_metrics(E, summary) -> None:
    for k in E.METRICS:
        if k in summary:
            s = summary[k]
            print(f"{k:12s} mean {s['mean']:.4f}  median {s['median']:.4f}  p95 {s['p95']:.4f}")


def copy_synthesis(parser, args, names, mels, pitch, energy, ref_waves) -> int:
    """--copy-synthesis: the cache's mels through the vocoder the flags name, against the recordings."""
    from kokoro.cli.synth import check_vocoder_model, load_vocoder
    from kokoro.inference import evaluate as E
    from kokoro_ruslan_amd.dtw import MelAligner
    device = torch.device("cuda")
    check_vocoder_model(parser, args, mels[0].shape[1])
    voc, vkw, den, how = load_vocoder(args, device)
    kw = dict(denoiser=den, denoise_strength=args.denoise) if den is not None else {}
    records, summary = E.evaluate_vocoder(voc, mels, ref_waves, pitch, energy, vocoder_kwargs=vkw, names=names, device=device,
                                          aligner=MelAligner(device=device, K=args.mcep, gpe_ratio=args.gpe_ratio), **kw)
    print(f"kokoro-eval: {summary['utterances']} utterances, copy synthesis; audio: {how}, {summary['no_variance']} without pitch and "
          f"energy in the cache")
    _print_metrics(E, summary)
    if args.output:
        with open(args.output, "w") as f:
            json.dump({"records": records, "summary": summary, "copy_synthesis": True, "audio": how, "gpe_ratio": args.gpe_ratio,
                       "wavs": args.wavs, "split": "indices" if args.indices is not None else (args.split or "val")}, f, indent=1)
        print(f"kokoro-eval: report -> {args.output}")
    return 0


def select_indices(n: int, split: Optional[str], validation_split: float, indices: Optional[List[int]]) -> List[int]:
    """Utterances of an n-utterance cache (length-sorted order): --indices as given, else the trainer's split."""
    if indices is not None:
        return list(indices)
    from kokoro.data.cached import split_indices
    if split == "all":
        return list(range(n))
    train, val = split_indices(n, validation_split)
    return train if split == "train" else val


def read_features(cache_dir: str, split: Optional[str], validation_split: float, indices: Optional[List[int]]):
    """(names, ids, stress, mels [T, M], durations, pitch [T], energy [T]) of the selected utterances."""
    from kokoro.data.cached import CachedFeatureDataset, scan_cache
    metas = scan_cache(cache_dir)
    sel = select_indices(len(metas), split or "val", validation_split, indices)
    ds = CachedFeatureDataset(cache_dir, indices=sel, memory_cache=False, metas=metas)
    names, ids, stress, mels, durs, pitch, energy = [], [], [], [], [], [], []
    for i in range(len(ds)):
        it = ds[i]
        names.append(os.path.splitext(ds.samples[i]["file"].name)[0])
        ids.append(it["phoneme_indices"].to(torch.int64))
        stress.append(it["stress_indices"].to(torch.int64))
        mels.append(it["mel_spec"].t().contiguous().float())
        durs.append(it["phoneme_durations"].to(torch.int64))
        pitch.append(it["pitch"].float().reshape(-1))
        energy.append(it["energy"].float().reshape(-1))
    return names, ids, stress, mels, durs, pitch, energy


def oracle_prosody(names, ids, durs, pitch=None, energy=None):
    """One Prosody per utterance that forces the cache's durations; ValueError names an utterance that has none for its phonemes.
    With pitch and energy (--oracle-prosody: the cache's frame-level tracks) they are forced too, frame by frame; ValueError names
    an utterance whose tracks are all zero (a cache written with --no-variance)."""
    from kokoro_ruslan_amd.prosody import Prosody
    flag = "--oracle-durations" if pitch is None else "--oracle-prosody"
    out = []
    for i, (name, u, dur) in enumerate(zip(names, ids, durs)):
        if dur is None or dur.numel() != u.numel() or dur.numel() == 0 or bool((dur < 0).any()):
            raise ValueError(f"{flag}: utterance {name} has no durations for its {int(u.numel())} phonemes in the cache")
        if pitch is None:
            out.append(Prosody(durations=dur.to(torch.int64)).validate(int(u.numel())))
            continue
        if not bool((pitch[i] != 0).any()) and not bool((energy[i] != 0).any()):
            raise ValueError(f"{flag}: utterance {name} has no pitch and energy in the cache (written with --no-variance)")
        out.append(Prosody.from_tracks(dur, pitch[i].clamp(0.0, 1.0), energy[i].clamp(0.0, 1.0)).validate(int(u.numel())))
    return out


class KeptScores:
    """A PhoneAligner's score() whose results stay for --pronunciation-tokens: evaluate() scores the synthesis first, then the recordings."""

    def __init__(self, aligner):
        self.aligner, self.calls = aligner, []

    def score(self, *args, **kwargs):
        self.calls.append(self.aligner.score(*args, **kwargs))
        return self.calls[-1]


def phone_scoring(args, device, n_classes: int, mels, ids):
    """(evaluate()'s phone_model / phone_aligner / optional_ids, how the model came about) for --pronunciation: the model of the file,
    or one fitted on the selection's cached mels.  ValueError names a model of another K or class count, or a phoneme id out of range."""
    from kokoro_ruslan_amd.align import PhoneAligner
    opt = list(getattr(args, "optional_id", []))
    if any(o >= n_classes for o in opt):
        raise ValueError(f"--optional-id must be a phoneme id below the checkpoint's {n_classes}")
    S = PhoneAligner.file_states(args.pronunciation) if args.pronunciation else getattr(args, "align_states", 1)
    M = PhoneAligner.file_mixtures(args.pronunciation) if args.pronunciation else getattr(args, "align_mixtures", 1)
    al = PhoneAligner(device=device, n_classes=n_classes, **({"states": S} if S > 1 else {}), **({"mixtures": M} if M > 1 else {}))
    if args.pronunciation:
        model, how = al.load(args.pronunciation), f"model {args.pronunciation}"
    else:
        model, _, scores = al.fit(mels, ids, opt, iters=getattr(args, "align_iters", 6))
        how = f"fitted on the selection in {len(scores)} passes"
    return dict(phone_model=model, phone_aligner=KeptScores(al), optional_ids=opt), how


def token_lists(rec) -> Optional[dict]:
    """The per-token tensors of a PhoneAligner.score record as JSON lists (None for a token without frames, or an infeasible utterance)."""
    if rec["tokens"] is None:
        return None
    t = rec["tokens"]
    return {"frames": t["frames"].tolist(), "hits": t["hits"].tolist(),
            "gop": [None if math.isnan(v) else v for v in t["gop"].tolist()],
            "logpost": [None if math.isnan(v) else v for v in t["logpost"].tolist()]}


def main(argv=None) -> int:
    from kokoro.inference import evaluate as E
    from kokoro.inference import synth as S
    parser, args = parse(argv)
    check_args(parser, args)
    audio = bool(args.vocoder or args.griffin_lim)
    names, ids, stress, mels, durs, pitch, energy = read_features(args.features, args.split, args.validation_split, args.indices)
    if not names:
        parser.error("the selection is empty: nothing to evaluate")
    ref_waves = None
    if hasattr(args, "wavs"):
        try:
            ref_waves = read_wavs(args.wavs, names)
        except ValueError as e:
            print(f"kokoro-eval: {e}", file=sys.stderr)
            return 1
    if getattr(args, "copy_synthesis", False):
        return copy_synthesis(parser, args, names, mels, pitch, energy, ref_waves)
    engine, controls, used = S.load_for_inference(args.checkpoint, weights=args.weights, math_mode=args.math, max_len=args.max_len,
                                                  stop_threshold=args.stop_threshold, min_len_ratio=args.min_len_ratio,
                                                  min_len_floor=args.min_len_floor)
    if engine.dims.mel != mels[0].shape[1]:
        parser.error(f"the checkpoint makes {engine.dims.mel} mel channels, the cache holds {mels[0].shape[1]}")
    pkw = {}
    if args.oracle_durations:
        try:
            pkw["prosody"] = oracle_prosody(names, ids, durs, *((pitch, energy) if getattr(args, "oracle_prosody", False) else ()))
        except ValueError as e:
            parser.error(str(e))
    how = ""
    if audio:
        from kokoro.cli.synth import check_vocoder_model, load_vocoder
        from kokoro_ruslan_amd.dtw import MelAligner
        check_vocoder_model(parser, args, engine.dims.mel)
        voc, vkw, den, how = load_vocoder(args, engine.device)
        pkw.update(vocoder=voc, vocoder_kwargs=vkw, ref_pitch=pitch, ref_energy=energy,
                   aligner=MelAligner(device=engine.device, K=args.mcep, gpe_ratio=args.gpe_ratio))
        if den is not None:
            pkw.update(denoiser=den, denoise_strength=args.denoise)
        if ref_waves is not None:
            pkw.update(ref_waves=ref_waves)
    pron = None
    if hasattr(args, "pronunciation"):
        try:
            phone, pron = phone_scoring(args, engine.device, engine.dims.vocab, mels, ids)
        except (ValueError, OSError) as e:
            print(f"kokoro-eval: --pronunciation: {e}", file=sys.stderr)
            return 1
        pkw.update(phone)
    records, summary = E.evaluate(engine, ids, stress, mels, stream=not args.no_stream, slots=32 if args.slots is None else args.slots,
                                  batch_size=32 if args.batch_size is None else args.batch_size, durations=durs, names=names,
                                  mcep=args.mcep, **pkw, **controls.kwargs())
    print(f"kokoro-eval: {summary['utterances']} utterances ({used} weights, {controls}), "
          f"{100.0 * summary['hit_bound_share']:.1f} % ended at their generation bound"
          + (f"; audio: {how}, {summary['no_variance']} without pitch and energy in the cache" if audio else "")
          + (f"; pronunciation: {pron}, {summary['pron_infeasible']} that cannot be aligned" if pron else ""))
    _print_metrics(E, summary)
    if getattr(args, "pronunciation_tokens", False):
        syn, ref = pkw["phone_aligner"].calls
        for rec, s, r in zip(records, syn, ref):
            rec["pron_tokens"], rec["ref_pron_tokens"] = token_lists(s), token_lists(r)
    if args.output:
        with open(args.output, "w") as f:
            json.dump({"records": records, "summary": summary, "controls": controls.kwargs(), "weights": used, "mcep": args.mcep,
                       "split": "indices" if args.indices is not None else (args.split or "val"), "checkpoint": args.checkpoint,
                       **({"oracle_durations": True} if args.oracle_durations else {}),
                       **({"oracle_prosody": True} if getattr(args, "oracle_prosody", False) else {}),
                       **({"audio": how, "gpe_ratio": args.gpe_ratio} if audio else {}),
                       **({"wavs": args.wavs} if ref_waves is not None else {}),
                       **({"pronunciation": pron, "optional_ids": pkw["optional_ids"]} if pron else {})}, f, indent=1)
        print(f"kokoro-eval: report -> {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
