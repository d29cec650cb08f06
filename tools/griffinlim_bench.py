#!/usr/bin/env python3
"""Griffin-Lim throughput: GriffinLimVocoder.vocode on B = 1, 8, 32, 64 log-mels of 300 frames at 60 iterations (momentum 0.99, the
reference's random initial phases drawn on the CPU), against the same algorithm written with torch.stft / torch.istft
(griffinlim_torch) in fp32 on the same GPU on a [B, 513, 300] batch, and in fp32 on the host CPU one utterance at a time (what the
reference runs).  Prints mel frames per second and the fused iteration's achieved HBM bandwidth: per iteration a tile reads the
spectra of its frames and halo (513 x 8 bytes each), and per frame S (513 x 4) and rebuilt (513 x 8) are read and the next spectrum
and rebuilt (513 x 8 each) written.

    python tools/griffinlim_bench.py [frames=300] [iters=3] [--cpu-max-b 8] [--only-kernels B]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kokoro_ruslan_amd import griffinlim_torch as GT
from kokoro_ruslan_amd.griffinlim import N_BINS, GriffinLimVocoder, inverse_mel_matrix

args = [a for a in sys.argv[1:]]
only = int(args[args.index("--only-kernels") + 1]) if "--only-kernels" in args else 0
cpu_max_b = int(args[args.index("--cpu-max-b") + 1]) if "--cpu-max-b" in args else 8
pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
frames = int(pos[0]) if pos else 300
iters = int(pos[1]) if len(pos) > 1 else 3
N_ITER = 60


def timed(fn, sync=True):
    fn()
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def iter_bytes(voc, fr):
    t = voc.tiles(fr)
    f1 = torch.clamp(t[:, 2] + voc.tile_frames, max=t[:, 1])
    h0 = torch.clamp(torch.minimum(t[:, 2] - 3, t[:, 1] - 5), min=0)
    h1 = torch.clamp(f1 + 3, max=t[:, 1])
    return int((h1 - h0).sum()) * N_BINS * 8 + sum(fr) * N_BINS * (4 + 8 + 8 + 8)


g = torch.Generator().manual_seed(0)
pool = [(GT.harmonic_logmel(frames, seed=i, f0=90.0 + 2 * i).float()).cuda() for i in range(64)]
voc = GriffinLimVocoder()
if only:
    voc.vocode(pool[:only], n_iter=N_ITER)
    torch.cuda.synchronize()
    for _ in range(iters):
        voc.vocode(pool[:only], n_iter=N_ITER)
    torch.cuda.synchronize()
    sys.exit(0)

print(f"Griffin-Lim, {frames}-frame mels, {N_ITER} iterations, {iters} timed calls each")
res = {}
drawn = [torch.rand((N_BINS, frames), dtype=torch.complex64, generator=g) for _ in range(64)]
for B in (1, 8, 32, 64):
    dt = timed(lambda: voc.vocode(pool[:B], n_iter=N_ITER))
    # the device part alone, on phases drawn beforehand; the fused iterations: 60 minus 0 iterations (init, iSTFT, packing)
    dp = timed(lambda: voc.vocode(pool[:B], n_iter=N_ITER, angles=drawn[:B]))
    dp0 = timed(lambda: voc.vocode(pool[:B], n_iter=0, angles=drawn[:B]))
    per_it = (dp - dp0) / N_ITER
    res[B] = B * frames / dt
    print(f"kernels    B={B:<2d}: {dt * 1e3:9.2f} ms  {res[B]:10.0f} frames/s   (phases drawn beforehand: {dp * 1e3:8.2f} ms, "
          f"{B * frames / dp:9.0f} frames/s; one iteration {per_it * 1e6:7.1f} us, {iter_bytes(voc, [frames] * B) / (B * frames) / 1024:.1f}"
          f" KiB/frame, {iter_bytes(voc, [frames] * B) / per_it / 1e9:6.0f} GB/s)")

pinv = inverse_mel_matrix().float().cuda()


def torch_gpu(B):
    mel = torch.stack(pool[:B])
    S = torch.relu(pinv @ torch.exp(mel).transpose(1, 2)).pow(0.5)                  # [B, 513, T]
    ang = torch.rand((B, N_BINS, frames), dtype=torch.complex64, generator=g).cuda()
    return GT.griffinlim(S, ang, N_ITER)


for B in (1, 8, 32, 64):
    dt = timed(lambda: torch_gpu(B))
    r = B * frames / dt
    print(f"torch GPU  B={B:<2d}: {dt * 1e3:9.2f} ms  {r:10.0f} frames/s   kernels / torch GPU = {res[B] / r:.2f}x")

cpu = [m.cpu() for m in pool]
for B in (1, 8, 32, 64):
    if B > cpu_max_b:
        break

    def torch_cpu():
        for m in cpu[:B]:
            S = GT.magnitude(m, torch.float32, solver="gels")
            GT.griffinlim(S, torch.rand((1, N_BINS, frames), dtype=torch.complex64)[0], N_ITER)
    dt = timed(torch_cpu, sync=False)
    r = B * frames / dt
    print(f"torch CPU  B={B:<2d}: {dt * 1e3:9.2f} ms  {r:10.0f} frames/s   kernels / torch CPU = {res[B] / r:.1f}x  "
          f"({torch.get_num_threads()} threads)")
