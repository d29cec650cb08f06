#!/usr/bin/env python3
"""What the audio metrics add to a free-running evaluation: evaluate() with and without a vocoder on the utterance mix of
tools/synth_stream_bench.py (256 utterances of 20-100 phonemes, 3 frames per phoneme, default model size, random weights, 32 slots),
against ground truths of 0.9-1.1 times the synthesized length with random pitch and energy tracks.  The vocoder is Griffin-Lim at 8
iterations and, when a generator checkpoint is given, HiFi-GAN as well.  Five repeats, every path interleaved inside every repeat
(same process, same clocks, same weights); prints per vocoder the median wall time of evaluate() without and with the audio metrics
and the split of the latter into synthesis / vocode / extract / align + track sums (each stage timed on its own on the same inputs),
then one JSON line.  The track kernel alone (kk_dtw_track_stats) is the difference of the align stage with and without tracks.

    python tools/eval_audio_bench.py [mode=bf16] [utterances=256] [repeats=5] [hifigan=PATH]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro.inference.audio import vocode
from kokoro.inference.evaluate import evaluate
from kokoro_ruslan_amd.dtw import MAX_FRAMES, MelAligner
from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.features import FeatureExtractor
from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
from kokoro_ruslan_amd.spec import ModelDims, StepHyper

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
HIFIGAN = sys.argv[4] if len(sys.argv) > 4 else None
SLOT_FRAMES = 512
KW = dict(max_len=SLOT_FRAMES, stop_threshold=0.0, min_len_ratio=1.0, min_len_floor=1, slot_frames=SLOT_FRAMES)
g = torch.Generator().manual_seed(0)
utts = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (N,), generator=g)]

e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=0)
DP = "duration_adaptor.variance_adaptor.duration_predictor.linear"
e.arena.P[DP + ".weight"].zero_()                              # log-duration = the bias alone: 3 frames per phoneme
e.arena.P[DP + ".bias"].fill_(1.4)
al, ex = MelAligner(), FeatureExtractor()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def track(n):
    """A normalised pitch track with unvoiced runs (about 40 % of the frames)."""
    p = 0.04 + 0.4 * torch.rand(n, generator=g)
    gate = torch.rand((n + 7) // 8, generator=g).repeat_interleave(8)[:n] < 0.4
    return p.masked_fill(gate, 0.0)


mels = e.generate_stream(utts, slots=32, **KW)                 # warm-up, and the lengths of the ground truths
refs, ref_pitch, ref_energy = [], [], []
for m in mels:
    T = max(1, int(m.shape[0] * float(torch.empty(1).uniform_(0.9, 1.1, generator=g))))
    refs.append(torch.randn(T, m.shape[1], generator=g).cuda() * 2 - 5)
    ref_pitch.append(track(T).cuda())
    ref_energy.append(torch.rand(T, generator=g).cuda())

vocoders = {"griffin_lim_8": (GriffinLimVocoder(), lambda: dict(n_iter=8, generator=torch.Generator().manual_seed(1)))}
if HIFIGAN:
    from kokoro_ruslan_amd.vocoder import HifiganVocoder
    vocoders["hifigan_bf16"] = (HifiganVocoder.from_checkpoint(HIFIGAN, None, device="cuda", math_mode="bf16"), dict)


def with_audio(voc, kwargs):
    return evaluate(e, utts, None, refs, slots=32, aligner=al, vocoder=voc, vocoder_kwargs=kwargs(), extractor=ex, ref_pitch=ref_pitch,
                    ref_energy=ref_energy, **KW)


result = {"mode": mode, "utterances": N, "repeats": REPEATS, "frames": sum(m.shape[0] for m in mels), "vocoders": {}}
evaluate(e, utts, None, refs, slots=32, aligner=al, **KW)      # warm-up of every path: workspaces at their final sizes
for name, (voc, kwargs) in vocoders.items():
    with_audio(voc, kwargs)
    result["vocoders"][name] = {k: [] for k in ("evaluate_mel_s", "evaluate_audio_s", "synth_s", "vocode_s", "extract_s", "align_s", "align_tracks_s")}
for _ in range(REPEATS):
    for name, (voc, kwargs) in vocoders.items():
        r = result["vocoders"][name]
        r["evaluate_mel_s"].append(timed(lambda: evaluate(e, utts, None, refs, slots=32, aligner=al, **KW))[1])
        r["evaluate_audio_s"].append(timed(lambda: with_audio(voc, kwargs))[1])
        mels, t = timed(lambda: e.generate_stream(utts, slots=32, want_info=True, **KW)[0])
        r["synth_s"].append(t)
        audio, t = timed(lambda: vocode(voc, mels, **kwargs()))
        r["vocode_s"].append(t)
        feats, t = timed(lambda: ex.extract(audio, max_seq_length=MAX_FRAMES + 1))
        r["extract_s"].append(t)
        tracks = {"pitch": ([f["pitch"] for f in feats], ref_pitch), "energy": ([f["energy"] for f in feats], ref_energy)}
        r["align_s"].append(timed(lambda: al.align(mels, refs))[1])
        r["align_tracks_s"].append(timed(lambda: al.align(mels, refs, tracks=tracks))[1])
print(f"{mode}: {N} utterances, {result['frames']} frames, 32 slots, {REPEATS} interleaved repeats")
for name, r in result["vocoders"].items():
    med = {k[:-2] + "_median_s": statistics.median(v) for k, v in list(r.items())}
    r.update(med, audio_over_mel=med["evaluate_audio_median_s"] / med["evaluate_mel_median_s"],
             track_stats_share=(med["align_tracks_median_s"] - med["align_median_s"]) / med["evaluate_audio_median_s"])
    ms = lambda k: f"{med[k + '_median_s'] * 1e3:.1f} ms [{min(r[k + '_s']) * 1e3:.1f}, {max(r[k + '_s']) * 1e3:.1f}]"
    print(f"  {name}: evaluate() on the mel alone {ms('evaluate_mel')} | with the audio metrics {ms('evaluate_audio')} = x{r['audio_over_mel']:.2f} | "
          f"synthesis {ms('synth')} | vocode {ms('vocode')} | extract {ms('extract')} | align {ms('align')} | align + track sums {ms('align_tracks')} "
          f"(the track sums: {100 * r['track_stats_share']:.2f} % of the call)")
print(json.dumps(result))
