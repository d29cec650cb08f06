#!/usr/bin/env python3
"""What the prosody controls cost in the prefill of KokoroEngine.generate_batch (_prefill_rows: pad, encode, durations, expansion,
variance adaptor, cross-attention K|V; the packing of the controls on the host included), at B = 1, 8, 32 ragged utterances of 20..100
phonemes, default model size, random weights with the duration bias raised so that a phoneme gets ~5 frames, bf16 mode:

  none         prosody=None: no prosody kernel is launched
  per-phoneme  scale, shift and forced per-phoneme pitch / energy: kk_prosody_durations + kk_prosody_variance
  contour      a frame-level pitch and energy track per utterance on the model's own durations (Prosody.from_tracks,
               force_durations=False): kk_prosody_durations + kk_prosody_contour

All three expand by the same durations, so the frames are the same.  Five repeats, the three interleaved per batch size; prints the
medians (ms per prefill) and the differences to `none`.

    python tools/prosody_bench.py [iters=20]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.prosody import Prosody
from kokoro_ruslan_amd.spec import VA, ModelDims, StepHyper

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
REPEATS = 5
g = torch.Generator().manual_seed(0)
pool = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (32,), generator=g)]

e = KokoroEngine(ModelDims(), StepHyper(), math_mode="bf16", total_steps=100, seed=0)
e.arena.P[f"{VA}.duration_predictor.linear.bias"].fill_(1.8)


def prefill(utts, prosody):
    with torch.no_grad(), e._no_dropout():
        return e._prefill_rows("syn.", utts, None, [int(u.numel()) for u in utts], prosody=prosody)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


print(f"prosody controls in the prefill of generate_batch, {iters} timed prefills per repeat, medians of {REPEATS} interleaved repeats")
for B in (1, 8, 32):
    utts = pool[:B]
    dur, Tb, T, _, _ = prefill(utts, None)
    per_phoneme, contour = [], []
    for b, u in enumerate(utts):
        n = int(u.numel())
        d = dur[b, :n].cpu()
        per_phoneme.append(Prosody(pitch_scale=1.1, pitch_shift=0.02, energy_scale=0.9, pitch=torch.rand(n, generator=g), energy=torch.rand(n, generator=g)))
        S = int(d.sum())
        contour.append(Prosody.from_tracks(d, torch.rand(S, generator=g), torch.rand(S, generator=g), force_durations=False,
                                           pitch_scale=1.1, pitch_shift=0.02, energy_scale=0.9))
    assert prefill(utts, per_phoneme)[1] == Tb and prefill(utts, contour)[1] == Tb, "the same frames in all three"
    t0, t1, t2 = [], [], []
    for _ in range(REPEATS):
        t0.append(timed(lambda: prefill(utts, None), iters))
        t1.append(timed(lambda: prefill(utts, per_phoneme), iters))
        t2.append(timed(lambda: prefill(utts, contour), iters))
    m0, m1, m2 = (statistics.median(v) for v in (t0, t1, t2))
    print(f"B={B:<2d} ({sum(Tb):5d} frames, T = {T:4d}): none {m0 * 1e3:8.3f} ms   per-phoneme {m1 * 1e3:8.3f} ms ({(m1 - m0) * 1e3:+.3f})   "
          f"contour {m2 * 1e3:8.3f} ms ({(m2 - m0) * 1e3:+.3f}; to per-phoneme {(m2 - m1) * 1e3:+.3f})")
