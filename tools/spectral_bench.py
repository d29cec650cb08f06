#!/usr/bin/env python3
"""Throughput of the spectral distance kernel and its share of a free-running evaluation with recordings.

Part 1: SpectralDistance.run_packed (the peaks, the walk along the paths with three analysis windows per frame, the finish pass) at
B = 64 pairs of 300 x 300 and of 1600 x 1800 frames, against the same fifteen sums formed with torch ops on the same GPU: fp32
torch.stft of both packed sides with each of the three windows, gathers of the frames along the path, the sums in fp64.  The paths are
MelAligner's on random mels of those sizes (the metric only needs monotone paths with realistic repeats); the waveforms are noise of
256 T samples.  Five repeats with the two device paths interleaved inside every repeat; medians, with the spread.
Part 2: evaluate() with Griffin-Lim (8 iterations) and recordings at 32 slots on the utterance mix of tools/dtw_bench.py: the time of
SpectralDistance.measure on that call's waveforms and paths, and its share of the call.  One JSON line at the end.

    python tools/spectral_bench.py [mode=bf16] [utterances=128] [repeats=5]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import features_torch as FT
from kokoro_ruslan_amd import spectral_torch as R
from kokoro_ruslan_amd.dtw import MelAligner
from kokoro_ruslan_amd.spectral import SpectralDistance
from kokoro_ruslan_amd.stft import HOP, N_FFT

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 128
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SIZES, B, M = ((300, 300), (1600, 1800)), 64, 80
al, sd = MelAligner(), SpectralDistance()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def torch_sums(wa, wb, path, poff, steps):
    """sums fp64 [15, B] with torch ops on the device: per pair and window an fp32 torch.stft of each side, gathers along the path."""
    out = torch.zeros(15, len(wa), dtype=torch.float64, device="cuda")
    for b, (a, r) in enumerate(zip(wa, wb)):
        p = path[poff[b]:poff[b] + steps[b]].long()
        a, r = a / (a.abs().max() + 1e-9), r / (r.abs().max() + 1e-9)
        for k, w in enumerate(R.WINDOWS):
            win = torch.hann_window(w, periodic=True, device="cuda")
            PA, PB = ((lambda X: (X.real ** 2 + X.imag ** 2).double())(torch.stft(x, N_FFT, HOP, w, win, center=True, pad_mode="reflect",
                                                                              onesided=True, return_complex=True)) for x in (a, r))
            PA, PB = PA[:, p[:, 0]], PB[:, p[:, 1]]
            d = 10.0 * torch.log10((PA + 1e-9) / (PB + 1e-9))
            out[5 * k:5 * k + 5, b] = torch.stack([(PA * PB).sqrt().sum(), PA.sum(), PB.sum(), d.sum(), (d * d).sum()])
    return out


result = {"mode": mode, "repeats": REPEATS, "spectral": {}, "evaluate": {}}
cases = {}
for Ta, Tb in SIZES:
    g = torch.Generator().manual_seed(Ta)
    syn = [(torch.randn(Ta, M, generator=g) * 2 - 5).cuda() for _ in range(B)]
    ref = [(s[torch.linspace(0, Ta - 1, Tb).round().long().cuda()] + 0.1 * torch.randn(Tb, M, generator=g).cuda()) for s in syn]
    run = al.run_packed(syn, ref)
    wa = [torch.randn(HOP * Ta, generator=g).cuda() for _ in range(B)]
    wb = [torch.randn(HOP * Tb, generator=g).cuda() for _ in range(B)]
    args = (wa, wb, run["path"], run["poff_host"], run["steps"], [Ta] * B, [Tb] * B)
    steps = run["steps"].tolist()
    ours = sd.run_packed(*args)["sums"]                          # warm-up, and the agreement of the two device paths
    base = torch_sums(wa, wb, run["path"], run["poff_host"], steps)
    gap = float(((ours - base).abs() / base.abs()).max())
    print(f"{Ta} x {Tb}, B = {B}: {sum(steps)} steps; kernel against torch ops, largest relative difference of the sums {gap:.2e}")
    cases[(Ta, Tb)] = (args, steps, {"kernel_s": [], "torch_s": [], "sums_rel_gap": gap, "steps": sum(steps)})
for _ in range(REPEATS):
    for key, (args, steps, r) in cases.items():
        r["kernel_s"].append(timed(lambda: sd.run_packed(*args))[1])
        r["torch_s"].append(timed(lambda: torch_sums(args[0], args[1], args[2], args[3], steps))[1])
for (Ta, Tb), (args, steps, r) in cases.items():
    tk, tt = statistics.median(r["kernel_s"]), statistics.median(r["torch_s"])
    r.update(kernel_median_s=tk, torch_median_s=tt, pairs_per_s=B / tk, steps_per_s=r["steps"] / tk)
    result["spectral"][f"{Ta}x{Tb}"] = r
    print(f"{Ta} x {Tb}, B = {B}: kernel {tk * 1e3:8.2f} ms [{min(r['kernel_s']) * 1e3:.2f}, {max(r['kernel_s']) * 1e3:.2f}] = {B / tk:7.0f} pairs/s = "
          f"{r['steps'] / tk / 1e6:5.2f} M steps/s | torch ops {tt * 1e3:8.1f} ms [{min(r['torch_s']) * 1e3:.1f}, {max(r['torch_s']) * 1e3:.1f}]")

# ---- part 2: the spectral distance's share of an evaluate() call ----------------------------------------------------------------
from kokoro.inference.evaluate import evaluate
from kokoro_ruslan_amd.engine import KokoroEngine
from kokoro_ruslan_amd.features import FeatureExtractor
from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
from kokoro_ruslan_amd.spec import ModelDims, StepHyper

SLOT_FRAMES = 512
KW = dict(max_len=SLOT_FRAMES, stop_threshold=0.0, min_len_ratio=1.0, min_len_floor=1, slot_frames=SLOT_FRAMES)
g = torch.Generator().manual_seed(0)
utts = [torch.randint(1, 59, (int(n),), generator=g).cuda() for n in torch.randint(20, 101, (N,), generator=g)]
e = KokoroEngine(ModelDims(), StepHyper(), math_mode=mode, total_steps=100, seed=0)
DP = "duration_adaptor.variance_adaptor.duration_predictor.linear"
e.arena.P[DP + ".weight"].zero_()                              # log-duration = the bias alone: 3 frames per phoneme
e.arena.P[DP + ".bias"].fill_(1.4)
mels = e.generate_stream(utts, slots=32, **KW)                 # warm-up
refs = [torch.randn(max(5, int(m.shape[0] * float(torch.empty(1).uniform_(0.9, 1.1, generator=g)))), m.shape[1], generator=g).cuda() * 2 - 5
        for m in mels]
waves = [FT.test_signal(HOP * r.shape[0], seed=k).float().cuda() for k, r in enumerate(refs)]
tracks = [torch.rand(r.shape[0], generator=g) for r in refs]
AKW = dict(slots=32, aligner=al, vocoder=GriffinLimVocoder(), vocoder_kwargs=dict(n_iter=8), extractor=FeatureExtractor(), ref_pitch=tracks,
           ref_energy=tracks, ref_waves=waves, spectral=sd, **KW)
_, _, audio = evaluate(e, utts, None, refs, want_audio=True, **AKW)
paths = [a["path"] for a in al.align(mels, refs, want_path=True)]
na, nb = [int(m.shape[0]) for m in mels], [int(r.shape[0]) for r in refs]
ev = {"spectral_s": [], "evaluate_s": []}
for _ in range(REPEATS):
    ev["spectral_s"].append(timed(lambda: sd.measure(audio, waves, paths, na, nb))[1])
    ev["evaluate_s"].append(timed(lambda: evaluate(e, utts, None, refs, **AKW))[1])
tsp, te = statistics.median(ev["spectral_s"]), statistics.median(ev["evaluate_s"])
ev.update(utterances=N, frames=sum(na), spectral_median_s=tsp, evaluate_median_s=te, spectral_share=tsp / te)
result["evaluate"] = ev
print(f"evaluate with Griffin-Lim (8 iterations) and recordings, {mode}, 32 slots: {N} utterances, {sum(na)} frames: spectral distance "
      f"{tsp * 1e3:.1f} ms [{min(ev['spectral_s']) * 1e3:.1f}, {max(ev['spectral_s']) * 1e3:.1f}] | evaluate {te * 1e3:.1f} ms | its share "
      f"{100 * tsp / te:.1f} %")
print(json.dumps(result))
