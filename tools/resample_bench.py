#!/usr/bin/env python3
"""Resampling throughput: Resampler.speed_perturb and FeatureExtractor.extract_perturbed on B = 1, 8, 32, 64 waveforms of about 300
frames with factors drawn as in training (1 + uniform(-0.1, 0.1): 22050 -> int(22050 f), mostly coprime rates).  Prints input samples
per second and milliseconds per call with the waveforms already on the device, the device time of the launches alone (events around
the calls), and the resample launch's share of an extract_perturbed call's device time.

    python tools/resample_bench.py [frames=300] [iters=20] [--only-kernels B]

--only-kernels B runs extract_perturbed on B waveforms and nothing else: the run to put under rocprofv3 --kernel-trace --stats."""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import features_torch as FT
from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.features import FeatureExtractor
from kokoro_ruslan_amd.resample import Resampler

args = [a for a in sys.argv[1:]]
only = int(args[args.index("--only-kernels") + 1]) if "--only-kernels" in args else 0
pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 20
WARMUP = 3


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def device_ms(fn):
    kk.profile_start()
    for _ in range(iters):
        fn()
    per = {}
    for name, _, ms in kk.profile_stop():
        per[name] = per.get(name, 0.0) + ms / iters
    return per


rng = random.Random(0)
host = [FT.test_signal(256 * (frames - 1) + 17 * i, seed=i, f0=90.0 + 5 * i).float() for i in range(64)]
pool = [w.cuda() for w in host]
factors = [1.0 + rng.uniform(-0.1, 0.1) for _ in range(64)]
rs, ext = Resampler(), FeatureExtractor()
if only:
    for _ in range(WARMUP + iters):
        ext.extract_perturbed(pool[:only], factors[:only])
    torch.cuda.synchronize()
    sys.exit(0)

print(f"speed perturbation, ~{frames}-frame waveforms, {iters} timed calls each after {WARMUP} warm-up calls")
for B in (1, 8, 32, 64):
    n = sum(w.shape[0] for w in host[:B])
    dt = timed(lambda: rs.speed_perturb(pool[:B], factors[:B]))
    per = device_ms(lambda: rs.speed_perturb(pool[:B], factors[:B]))
    print(f"speed_perturb     B={B:<2d}: {dt * 1e3:8.3f} ms  {n / dt:12.0f} samples/s   (launches {sum(per.values()):7.3f} ms: "
          + ", ".join(f"{k[3:]} {v:.3f}" for k, v in per.items()) + ")")
    dt = timed(lambda: ext.extract_perturbed(pool[:B], factors[:B]))
    per = device_ms(lambda: ext.extract_perturbed(pool[:B], factors[:B]))
    dev = sum(per.values())
    print(f"extract_perturbed B={B:<2d}: {dt * 1e3:8.3f} ms  {n / dt:12.0f} samples/s   (launches {dev:7.3f} ms, resample "
          f"{per.get('kk_resample', 0.0):.3f} ms = {100 * per.get('kk_resample', 0.0) / dev:4.1f} % of them: "
          + ", ".join(f"{k[3:]} {v:.3f}" for k, v in per.items()) + ")")
