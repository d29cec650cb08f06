#!/usr/bin/env python3
"""Long-form synthesis, the two device stages against what they replace, on B = 1, 8, 32, 64 chunks of 300 frames:

  finish   kokoro.inference.audio.finish_mels (one launch, one host read) against the present path of kokoro-synth --trim: every mel to
           the host, kokoro.inference.synth.trim_trailing_silence there (two quantiles and a nonzero per mel), and the trimmed mel back
           to the device for the vocoder.
  join     kokoro_ruslan_amd.longform.join of the B chunk waveforms (300 x 256 samples each) into one document with 3307-sample gaps
           against torch.cat of the chunks and torch.zeros(3307) on the device, plus the per-chunk abs().max() both deliver.

Five repeats, the two paths interleaved per batch size; prints the medians (ms per call) and the ratios, after checking that both
paths keep the same frames and build the same document.

    python tools/longform_bench.py [frames=300] [iters=20]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro.inference.audio import finish_mels
from kokoro.inference.synth import trim_trailing_silence
from kokoro_ruslan_amd.longform import MelFinisher, join

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 20
REPEATS, GAP = 5, 3307
n = frames * 256


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def speechlike(g, i):
    """voiced frames, then 25 % + i frames of near-silence: the trim has something to cut"""
    voiced = frames - frames // 4 - i
    means = torch.cat([-6.0 + 3.0 * torch.rand(voiced, generator=g), -10.95 + 0.3 * torch.rand(frames - voiced, generator=g)])
    return means[:, None] + 0.8 * (torch.rand(frames, 80, generator=g) - 0.5)


def host_path(mels):
    return [trim_trailing_silence(m.float().cpu()).cuda() for m in mels]


def cat_path(waves):
    silence = torch.zeros(GAP, device="cuda")
    parts = []
    for k, w in enumerate(waves):
        parts += ([silence] if k else []) + [w]
    return torch.cat(parts), torch.stack([w.abs().max() for w in waves])


g = torch.Generator().manual_seed(0)
mel_pool = [speechlike(g, i).cuda() for i in range(64)]
wave_pool = [(0.1 * torch.randn(n, generator=g)).cuda() for _ in range(64)]
fin = MelFinisher()

print(f"long-form stages, chunks of {frames} frames / {n} samples, {iters} timed calls per repeat, medians of {REPEATS} interleaved repeats")
for B in (1, 8, 32, 64):
    mels, waves = mel_pool[:B], wave_pool[:B]
    assert all(torch.equal(a, b) for a, b in zip(finish_mels(fin, mels)[0], host_path(mels)))
    (doc,), peaks = join(waves, [list(range(B))], GAP)
    want, want_peaks = cat_path(waves)
    assert torch.equal(doc, want) and torch.equal(peaks, want_peaks)
    ours, theirs, jo, jt = [], [], [], []
    for _ in range(REPEATS):
        ours.append(timed(lambda: finish_mels(fin, mels), iters))
        theirs.append(timed(lambda: host_path(mels), iters))
        jo.append(timed(lambda: join(waves, [list(range(B))], GAP), iters))
        jt.append(timed(lambda: cat_path(waves), iters))
    do, dt, djo, djt = (statistics.median(v) for v in (ours, theirs, jo, jt))
    print(f"B={B:<2d}: finish_mels {do * 1e3:8.3f} ms   host trim per mel {dt * 1e3:8.3f} ms   device / host = {dt / do:5.1f}x   |   "
          f"join {djo * 1e3:8.3f} ms  {B * n * 8 / djo / 1e9:7.1f} GB/s   torch.cat + peaks {djt * 1e3:8.3f} ms   join / cat = {djt / djo:5.1f}x")
