#!/usr/bin/env python3
"""Loudness-normalisation throughput: LoudnessNormaliser.normalise (trim at 40 dB, -23 LUFS, -1 dB peak) on B = 1, 8, 32, 64 waveforms
of 300 x 256 samples, against the fp64 oracle (kokoro_ruslan_amd.loudness_torch.normalise) on the host in 16 threads, one waveform
after the other.  Five repeats, the two interleaved per batch size; prints the medians (ms per call, samples per second), the ratio and
the largest loudness difference between the two.

    python tools/loudness_bench.py [frames=300] [iters=20]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import loudness_torch as LT
from kokoro_ruslan_amd.loudness import LoudnessNormaliser

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 20
REPEATS, HOST_THREADS = 5, 16
n = frames * 256
torch.set_num_threads(HOST_THREADS)


def timed(fn, sync, reps):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


g = torch.Generator().manual_seed(0)
env = torch.ones(n)
env[:n // 10] = 1e-4
env[-n // 8:] = 1e-4
host = [(0.02 + 0.004 * i) * torch.randn(n, generator=g) * env for i in range(64)]
pool = [w.cuda() for w in host]
norm = LoudnessNormaliser()

print(f"loudness normalisation with trim, {frames} x 256-sample waveforms at 22050 Hz, {iters} timed calls per repeat on the device "
      f"(1 on the host), medians of {REPEATS} interleaved repeats")
for B in (1, 8, 32, 64):
    waves, cpu = pool[:B], host[:B]
    info = norm.normalise(waves, trim_db=40.0)[1]
    want = [LT.normalise(w, trim=40.0)[1] for w in cpu]
    assert all((a["start"], a["end"]) == (b["start"], b["end"]) for a, b in zip(info, want))
    dL = max(abs(a["measured"] - b["measured"]) for a, b in zip(info, want))
    ours, theirs = [], []
    for _ in range(REPEATS):
        ours.append(timed(lambda: norm.normalise(waves, trim_db=40.0), torch.cuda.synchronize, iters))
        theirs.append(timed(lambda: [LT.normalise(w, trim=40.0) for w in cpu], lambda: None, 1))
    do, dt = statistics.median(ours), statistics.median(theirs)
    print(f"B={B:<2d}: kernels {do * 1e3:8.3f} ms  {B * n / do / 1e6:9.1f} M samples/s   fp64 oracle, host {dt * 1e3:9.3f} ms  "
          f"{B * n / dt / 1e6:9.1f} M samples/s   kernels / host = {dt / do:.1f}x   (largest |dL| {dL:.1e} LU)")
