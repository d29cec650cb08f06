#!/usr/bin/env python3
"""Feature-extraction throughput: FeatureExtractor.extract on B = 1, 8, 32, 64 waveforms of about 300 frames (log-mel, pitch and energy),
against the same contract written with torch.stft / torch.fft (features_torch) in fp32 on the same GPU one utterance at a time (its
statistics are per utterance) and in fp32 on the host CPU (what the reference runs).  Prints mel frames per second for a call with the
waveforms already on the device, for a call that starts from host tensors (packing and upload included), and the device time of the
four launches alone (events around the calls).

    python tools/features_bench.py [frames=300] [iters=20] [--cpu-max-b 8] [--only-kernels B]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import features_torch as FT
from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.features import FeatureExtractor

args = [a for a in sys.argv[1:]]
only = int(args[args.index("--only-kernels") + 1]) if "--only-kernels" in args else 0
cpu_max_b = int(args[args.index("--cpu-max-b") + 1]) if "--cpu-max-b" in args else 8
pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 20
WARMUP = 3


def timed(fn, sync=True, n=None):
    n = n or iters
    for _ in range(WARMUP):
        fn()
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


host = [FT.test_signal(256 * (frames - 1) + 17 * i, seed=i, f0=90.0 + 5 * i).float() for i in range(64)]
pool = [w.cuda() for w in host]
nframes = lambda B: sum(FT.mel_frames(w.shape[0]) for w in host[:B])
ext = FeatureExtractor()
if only:
    for _ in range(WARMUP + iters):
        ext.extract(pool[:only])
    torch.cuda.synchronize()
    sys.exit(0)

print(f"feature extraction, ~{frames}-frame waveforms, {iters} timed calls each after {WARMUP} warm-up calls")
res = {}
for B in (1, 8, 32, 64):
    dt = timed(lambda: ext.extract(pool[:B]))
    dh = timed(lambda: ext.extract(host[:B]))
    kk.profile_start()
    for _ in range(iters):
        ext.extract(pool[:B])
    rec = kk.profile_stop()
    per = {}
    for name, _, ms in rec:
        per[name] = per.get(name, 0.0) + ms / iters
    dev = sum(per.values())
    res[B] = nframes(B) / dt
    print(f"kernels    B={B:<2d}: {dt * 1e3:8.3f} ms  {res[B]:10.0f} frames/s   (from host tensors {dh * 1e3:8.3f} ms; the four launches "
          f"{dev:7.3f} ms = {100 * dev / (dt * 1e3):4.1f} % of the call: " + ", ".join(f"{k[8:]} {v:.3f}" for k, v in per.items()) + ")")

for B in (1, 8, 32, 64):
    dt = timed(lambda: [FT.extract(w, dtype=torch.float32) for w in pool[:B]], n=max(iters // 4, 2))
    r = nframes(B) / dt
    print(f"torch GPU  B={B:<2d}: {dt * 1e3:8.3f} ms  {r:10.0f} frames/s   kernels / torch GPU = {res[B] / r:.2f}x")

for B in (1, 8, 32, 64):
    if B > cpu_max_b:
        break
    dt = timed(lambda: [FT.extract(w, dtype=torch.float32) for w in host[:B]], sync=False, n=max(iters // 4, 2))
    r = nframes(B) / dt
    print(f"torch CPU  B={B:<2d}: {dt * 1e3:8.3f} ms  {r:10.0f} frames/s   kernels / torch CPU = {res[B] / r:.1f}x  "
          f"({torch.get_num_threads()} threads)")
