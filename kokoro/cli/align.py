"""`kokoro-align`: phoneme durations for a feature cache by flat-start forced alignment on the device (no external aligner).

    kokoro-align --cache-dir DIR [--iters N] [--optional-id ID ...] [--batch-size N] [--var-floor F] [--mcep K] [--n-classes V]
                 [--model-in FILE | --model-out FILE] [--output FILE.jsonl] [--write-cache] [--scores [--worst N]] [--states S]
                 [--mixtures M [--mix-iters N]]

Reads the schema-v7 entries of a feature cache (mel_spec, phoneme_indices), fits one diagonal Gaussian per phoneme id by Viterbi
training from the even split (kokoro_ruslan_amd.align.PhoneAligner.fit) -- or, with --model-in, loads a fitted model and only aligns --
and gives every utterance the durations of its best path: frames per phoneme, summing to mel_length.  --optional-id names phoneme ids
whose tokens may get no frame (a silence the speaker did not make; there is no default: the id of <sil> is the vocabulary's business).
--output writes one {"name", "phoneme_durations"} line per utterance, the field kokoro-precompute --ids accepts; --write-cache replaces
phoneme_durations in every entry, atomically.  An utterance that cannot be aligned (more mandatory tokens than frames, or longer than
the kernels take) keeps the durations it has, is reported on stderr and makes the exit status 1.
--scores (after a fit or with --model-in) also scores every utterance against its own transcript with the model
(PhoneAligner.score): gop, the mean over the frames of log-likelihood(forced phoneme) - log-likelihood(best phoneme); logpost, the mean
log posterior of the forced phoneme; phone_acc, the share of frames whose best phoneme is the forced one; gop_min and gop_min_token,
the worst token and where it is.  The five fields join every --output line (null for an utterance that was not aligned) and the
--worst N (default 10) utterances by gop are printed, lowest first: where a transcript does not match its audio, the scores fall.  They
rank; no threshold says "wrong".
--states S (1, 2 or 3; default 1) gives every phoneme a left-to-right chain of S states with a Gaussian each: a phone is a closure and
a burst, an onset and an offset, and a token that has frames then has at least S of them (at a 11.6 ms hop S = 3 means >= 35 ms per
phone, which is why 1 stays the default; a present optional silence needs >= S frames too, so a shorter pause falls to its
neighbours).  With --model-in the file's value holds (a conflicting --states is named, exit status 1).  With S > 1 the --output lines
gain "state_durations" ([P][S], rows summing to phoneme_durations; null where the utterance was not aligned); --write-cache writes the
phone durations.
--mixtures M (1, 2 or 4; default 1) gives every state a mixture of M diagonal Gaussians (n-classes x states x M <= 1024): the
single-Gaussian training runs first as always, then every component is split in two and up to --mix-iters N passes (default 4) assign
every frame to the best component of its state and re-estimate, once for 2 and again for 4; one closing alignment gives the durations.
With --model-in the file's value holds (a conflicting --mixtures is named, exit status 1).  The output lines do not change.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List


SCORE_FIELDS = ("gop", "logpost", "phone_acc", "gop_min", "gop_min_token")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="kokoro-align", description=__doc__.split("\n\n")[0])
    p.add_argument("--cache-dir", required=True, metavar="DIR", help="feature cache (*.pt)")
    p.add_argument("--iters", type=int, default=6, help="passes of Viterbi training (default 6)")
    p.add_argument("--optional-id", type=int, action="append", default=[], metavar="ID", help="a phoneme id whose tokens may be skipped")
    p.add_argument("--batch-size", type=int, default=64, help="utterances per device call")
    p.add_argument("--var-floor", type=float, default=0.01, help="variance floor as a share of the global variance")
    p.add_argument("--mcep", type=int, default=13, metavar="K", help="cepstral coefficients c1..cK of the features (default 13)")
    p.add_argument("--n-classes", type=int, default=59, metavar="V", help="phoneme ids (default 59)")
    m = p.add_mutually_exclusive_group()
    m.add_argument("--model-in", metavar="FILE", help="align with this model instead of fitting one")
    m.add_argument("--model-out", metavar="FILE", help="save the fitted model")
    p.add_argument("--output", metavar="FILE.jsonl", default=None)
    p.add_argument("--write-cache", action="store_true", help="replace phoneme_durations in the cache entries")
    # (these leave no attribute behind when they are not given: an invocation without them parses as it always did)
    p.add_argument("--scores", action="store_true", default=argparse.SUPPRESS,
                   help="score every utterance against its transcript: gop, logpost, phone_acc, gop_min, gop_min_token")
    p.add_argument("--worst", type=int, default=argparse.SUPPRESS, metavar="N", help="with --scores: print the N utterances of lowest gop (default 10)")
    p.add_argument("--states", type=int, default=argparse.SUPPRESS, metavar="S",
                   help="states per phoneme, 1..3 (default 1; with --model-in the file's value)")
    p.add_argument("--mixtures", type=int, default=argparse.SUPPRESS, metavar="M",
                   help="Gaussians per state: 1, 2 or 4 (default 1; with --model-in the file's value)")
    p.add_argument("--mix-iters", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --mixtures 2 or 4: passes after each doubling of the components (default 4)")
    return p


def check_args(p: argparse.ArgumentParser, args) -> None:
    if args.iters < 1:
        p.error("--iters must be >= 1")
    if args.batch_size < 1:
        p.error("--batch-size must be >= 1")
    if not (0.0 <= args.var_floor < 1.0):
        p.error("--var-floor must be in [0, 1)")
    if not (0 <= args.mcep <= 31):
        p.error("--mcep must be in 0..31")
    if not (1 <= args.n_classes <= 256):
        p.error("--n-classes must be in 1..256")
    if any(not (0 <= o < args.n_classes) for o in args.optional_id):
        p.error("--optional-id must be a phoneme id below --n-classes")
    if hasattr(args, "worst") and not getattr(args, "scores", False):
        p.error("--worst needs --scores")
    if getattr(args, "worst", 10) < 0:
        p.error("--worst must be >= 0")
    if not (1 <= getattr(args, "states", 1) <= 3):
        p.error("--states must be 1, 2 or 3")
    if getattr(args, "mixtures", 1) not in (1, 2, 4):
        p.error("--mixtures must be 1, 2 or 4")
    if getattr(args, "mix_iters", 4) < 1:
        p.error("--mix-iters must be >= 1")
    if hasattr(args, "mix_iters") and (getattr(args, "mixtures", 1) == 1 or args.model_in):
        p.error("--mix-iters needs --mixtures 2 or 4 and a fit: not with --model-in")
    if args.n_classes * getattr(args, "states", 1) * getattr(args, "mixtures", 1) > 1024:
        p.error(f"--n-classes {args.n_classes} x --states {getattr(args, 'states', 1)} x --mixtures {getattr(args, 'mixtures', 1)} = "
                f"{args.n_classes * getattr(args, 'states', 1) * getattr(args, 'mixtures', 1)} Gaussians; at most 1024")
    if args.n_classes * getattr(args, "states", 1) > 256:
        p.error(f"--n-classes {args.n_classes} x --states {args.states} = {args.n_classes * args.states} Gaussians; at most 256")


def read_cache(cache_dir: str) -> List[Dict]:
    """[{"path", "name", "mel" [T, M], "ids" [P], "durations" [P]}] of the cache's entries, in its length-sorted order."""
    import torch
    from kokoro.data.cached import scan_cache
    out = []
    for meta in scan_cache(cache_dir):
        it = torch.load(meta["file"], map_location="cpu", weights_only=False)
        T = int(it["mel_length"])
        out.append({"path": str(meta["file"]), "name": os.path.splitext(meta["file"].name)[0],
                    "mel": it["mel_spec"][:, :T].t().contiguous().float(), "ids": it["phoneme_indices"].to(torch.int64),
                    "durations": it["phoneme_durations"].to(torch.int64)})
    return out


def replace_durations(path: str, durations) -> None:
    """Rewrite one cache entry with other phoneme_durations, atomically (as kokoro.data.features.write_cache_entry writes it)."""
    import torch
    it = torch.load(path, map_location="cpu", weights_only=False)
    it["phoneme_durations"] = durations.to(torch.long).contiguous()
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(it, tmp)
    os.replace(tmp, path)


def main(argv=None) -> int:
    p = build_parser()
    args = p.parse_args(argv)
    check_args(p, args)
    import torch
    from kokoro_ruslan_amd import align as A

    S, M = getattr(args, "states", 1), getattr(args, "mixtures", 1)
    if args.model_in:
        M = A.PhoneAligner.file_mixtures(args.model_in)
        if getattr(args, "mixtures", M) != M:
            print(f"kokoro-align: --mixtures {args.mixtures}, but {args.model_in} is a model of mixtures = {M}: leave --mixtures out, or fit "
                  "another model", file=sys.stderr)
            return 1
        S = A.PhoneAligner.file_states(args.model_in)
        if getattr(args, "states", S) != S:
            print(f"kokoro-align: --states {args.states}, but {args.model_in} is a model of states = {S}: leave --states out, or fit another "
                  "model", file=sys.stderr)
            return 1
        if args.n_classes * S > 256:
            p.error(f"{args.model_in}: states = {S}; --n-classes {args.n_classes} x {S} Gaussians are more than 256")
    entries = read_cache(args.cache_dir)
    al = A.PhoneAligner(K=args.mcep, n_classes=args.n_classes, var_floor=args.var_floor, **({"states": S} if S > 1 else {}),
                        **({"mixtures": M} if M > 1 else {}))
    limit = A.max_tokens()
    failed = 0
    todo = []
    for n, e in enumerate(entries):
        P, T = int(e["ids"].shape[0]), int(e["mel"].shape[0])
        why = (f"{T} frames; at most {A.MAX_FRAMES}" if T > A.MAX_FRAMES else f"{P} tokens; at most {limit}" if P > limit else
               "no tokens" if P < 1 else "no frames" if T < 1 else
               f"a phoneme id outside 0..{args.n_classes - 1}" if int(e["ids"].min()) < 0 or int(e["ids"].max()) >= args.n_classes else None)
        if why:
            failed += 1
            print(f"kokoro-align: {e['name']}: {why}; its durations stay", file=sys.stderr)
        else:
            todo.append(n)
    if not todo:
        p.error("no utterance of the cache can be aligned")
    mels, ids = [entries[n]["mel"] for n in todo], [entries[n]["ids"] for n in todo]
    want_scores = getattr(args, "scores", False)

    def batches(fn):
        return [r for s in range(0, len(todo), args.batch_size)
                for r in fn(mels[s:s + args.batch_size], ids[s:s + args.batch_size], args.optional_id, model)]
    if args.model_in:
        model = al.load(args.model_in)
        recs = batches(al.score if want_scores else al.align)
        durs, how = [r["durations"] for r in recs], f"model {args.model_in}"
        sdurs = [r["state_durations"] for r in recs] if S > 1 else None
        score = sum(r["score"] for r in recs if r["feasible"])
    else:
        model, durs, scores = al.fit(mels, ids, args.optional_id, iters=args.iters, batch_size=args.batch_size,
                                     **({"mix_iters": args.mix_iters} if hasattr(args, "mix_iters") else {}))
        how, score, sdurs = f"{len(scores)} passes", scores[-1], al.state_durations
        if args.model_out:
            al.save(model, args.model_out)
        recs = batches(al.score) if want_scores else None
    if want_scores:
        for n, r in zip(todo, recs):
            entries[n]["scores"] = {k: r[k] for k in SCORE_FIELDS}
    aligned = 0
    optional = torch.tensor(sorted(set(args.optional_id)), dtype=torch.int64)
    for k, (n, d) in enumerate(zip(todo, durs)):
        e = entries[n]
        if d is None:
            failed += 1
            need = S * int((~torch.isin(e["ids"], optional)).sum())
            if S > 1 and need > e["mel"].shape[0]:
                print(f"kokoro-align: {e['name']}: {e['ids'].shape[0]} tokens of {S} states need at least {need} frames and cannot be laid "
                      f"on {e['mel'].shape[0]}; its durations stay (a lower --states would need fewer)", file=sys.stderr)
                continue
            print(f"kokoro-align: {e['name']}: {e['ids'].shape[0]} tokens cannot be laid on {e['mel'].shape[0]} frames; its durations stay",
                  file=sys.stderr)
            continue
        aligned += 1
        e["durations"] = d
        if S > 1:
            e["state_durations"] = sdurs[k]
        if args.write_cache:
            replace_durations(e["path"], d)
    if args.output:
        with open(args.output, "w") as f:
            for e in entries:
                f.write(json.dumps({"name": e["name"], "phoneme_durations": [int(v) for v in e["durations"]],
                                    **(e.get("scores", dict.fromkeys(SCORE_FIELDS)) if want_scores else {}),
                                    **({"state_durations": e["state_durations"].tolist() if "state_durations" in e else None}
                                       if S > 1 else {})}) + "\n")
    frames = sum(int(entries[n]["mel"].shape[0]) for n, d in zip(todo, durs) if d is not None)
    print(f"kokoro-align: {aligned} aligned, {failed} infeasible ({len(entries)} utterances), {how}, "
          f"log-likelihood per frame {score / max(frames, 1):.4f}" + (" -> " + args.cache_dir if args.write_cache else ""))
    if want_scores:
        ranked = sorted((e for e in entries if e.get("scores", {}).get("gop") is not None), key=lambda e: e["scores"]["gop"])
        for e in ranked[:getattr(args, "worst", 10)]:
            s = e["scores"]
            print(f"kokoro-align: {e['name']}: gop {s['gop']:.4f}  logpost {s['logpost']:.4f}  phone_acc {s['phone_acc']:.3f}  "
                  f"gop_min {s['gop_min']:.4f} at token {s['gop_min_token']}")
    return 0 if failed == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
