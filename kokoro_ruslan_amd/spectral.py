"""The spectral distance of vocoded audio to the speaker's recording along the mels' DTW alignment, on the device, on the kernel of
csrc/kk_spectral.hip.

The mel metrics of an evaluation end at the decoder, and the F0 / voicing / energy errors of the vocoded audio do not move when a
vocoder's noise floor, the denoiser's strength or Griffin-Lim's iteration count change.  `SpectralDistance.measure` is the measurement
that does: for every pair (synthesized waveform, recording) and the path MelAligner found for their mels it walks the path, transforms
the two frames of each step with three analysis windows (256, 512, 1024 in one 1024-point fp64 transform) and keeps five fp64 sums per
window, from which come the spectral convergence at the least-squares gain, the level offset in dB and the log-spectral distance
with that offset taken out (the definitions and the fp64 oracle: spectral_torch.py).  The pairs of a call are packed and run through
one launch and its finish pass; a pair's sums are, bit for bit, what it gives alone.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.spectral_torch import MAX_STEPS, MIN_SAMPLES, WINDOWS, spectral_metrics
from kokoro_ruslan_amd.stft import N_FFT, centred_hann_windows

MAX_SAMPLES = (1 << 31) - 1 - MIN_SAMPLES


def tile_steps() -> int:
    """Path steps one workgroup of the kernel owns (its constant)."""
    return int(kk.load().kk_dtw_spectral_tile())


def _check_waves(what: str, waves: Sequence[torch.Tensor], B: int) -> None:
    if len(waves) != B:
        raise ValueError(f"{len(waves)} {what} waveforms for {B} pairs")
    for i, w in enumerate(waves):
        if not isinstance(w, torch.Tensor) or w.dim() != 1 or not w.is_floating_point():
            raise ValueError(f"pair {i}: the {what} waveform must be a 1-D float tensor")
        if w.numel() < MIN_SAMPLES or w.numel() > MAX_SAMPLES:
            raise ValueError(f"pair {i}: the {what} waveform has {w.numel()} samples, expected {MIN_SAMPLES} .. {MAX_SAMPLES}: the STFT "
                             f"reflect-pads {MIN_SAMPLES // 2} samples at each end")


def _check_frames(what: str, frames: Sequence[int], B: int) -> List[int]:
    if len(frames) != B:
        raise ValueError(f"{len(frames)} {what} frame counts for {B} pairs")
    out = []
    for i, t in enumerate(frames):
        if isinstance(t, bool) or int(t) != t or t < 1:
            raise ValueError(f"pair {i}: {what} frames must be an integer >= 1, not {t!r}")
        out.append(int(t))
    return out


class SpectralDistance:
    """measure(synthesized waveforms, recordings, DTW paths, mel frames of both sides) -> one record per pair."""

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        self.windows = centred_hann_windows(torch.float64).to(self.device).contiguous()      # fp64 tables: the kernel transforms in fp64
        ang = -2.0 * math.pi * torch.arange(N_FFT, dtype=torch.float64) / N_FFT
        self.tw = torch.stack([torch.cos(ang), torch.sin(ang)], 1).contiguous().to(self.device)
        self.tile = tile_steps()

    def measure(self, syn_waves: Sequence[torch.Tensor], ref_waves: Sequence[torch.Tensor], paths: Sequence[torch.Tensor],
                syn_frames: Sequence[int], ref_frames: Sequence[int]) -> List[Dict]:
        """Pair b: syn_waves[b] (vocoded from a mel of syn_frames[b] frames), ref_waves[b] (the recording; its mel has ref_frames[b]
        frames) and paths[b], an integer tensor [steps <= 8191, 2] of (i, j) in mel frames (MelAligner.align(want_path=True)).  Waveforms
        are 1-D float tensors of at least 1024 un-normalised samples at 22050 Hz, on any device.  Returns per pair the fields of
        spectral_torch.spectral_metrics: sc_dtw_W, lsd_dtw_W, level_db_W for W in 256, 512, 1024, mr_sc_dtw, mr_lsd_dtw, spec_steps and
        spec_skipped (steps whose index lies outside its mel or whose frame centre lies past its waveform: counted, never read).  One
        read by the host for the whole call."""
        B = len(paths)
        _check_waves("synthesized", syn_waves, B)
        _check_waves("reference", ref_waves, B)
        na, nb = _check_frames("synthesized", syn_frames, B), _check_frames("reference", ref_frames, B)
        for i, p in enumerate(paths):
            if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.shape[1] != 2 or p.is_floating_point() or p.dtype == torch.bool:
                raise ValueError(f"pair {i}: the path must be an integer tensor [steps, 2]")
            if not (1 <= p.shape[0] <= MAX_STEPS):
                raise ValueError(f"pair {i}: a path of {p.shape[0]} steps; expected 1 .. {MAX_STEPS}")
        if B == 0:
            return []
        n = [int(p.shape[0]) for p in paths]
        path = torch.cat([p.to(self.device, torch.int32) for p in paths]).contiguous()
        g = self.run_packed(syn_waves, ref_waves, path, kk.packed_offsets(n).tolist(), torch.tensor(n, dtype=torch.int32).to(self.device), na, nb)
        host = torch.cat([g["sums"], g["counts"].double()]).cpu().tolist()
        return [spectral_metrics([row[b] for row in host[:15]], int(host[15][b]), int(host[16][b])) for b in range(B)]

    def tiles(self, room: Sequence[int]):
        """(tiles int32 [ntiles, 2] = {pair, first step}, toff int32 [B + 1]) over the path entries each pair has room for."""
        per = [-(-r // self.tile) for r in room]
        tiles = torch.tensor([[b, t * self.tile] for b, k in enumerate(per) for t in range(k)], dtype=torch.int32).reshape(-1, 2)
        return tiles, kk.packed_offsets(per, torch.int32)

    def run_packed(self, syn_waves: Sequence[torch.Tensor], ref_waves: Sequence[torch.Tensor], path: torch.Tensor,
                   poff_host: Sequence[int], steps: torch.Tensor, syn_frames: Sequence[int], ref_frames: Sequence[int]) -> Dict:
        """One batch on the device, nothing read back.  path int32 [P, 2], poff_host (B + 1 first entries) and steps int32 [B] on the
        device are MelAligner.run_packed's "path", "poff_host" and "steps"; a pair is walked for min(steps[b], its room) entries.
        Arguments as measure() checks them.  Returns the device tensors sums fp64 [15, B] (row 5 w + {0: sum AB, 1: sum A^2,
        2: sum B^2, 3: sum d, 4: sum d^2}, w the window), counts int32 [2, B] (counted, skipped) and peaks fp32 [2, B]."""
        dev, B = self.device, len(syn_waves)
        if len(poff_host) != B + 1 or B < 1:
            raise ValueError(f"poff_host: {len(poff_host)} entries for {B} pairs (B + 1 expected, B >= 1)")
        room = [int(poff_host[b + 1]) - int(poff_host[b]) for b in range(B)]
        if int(poff_host[0]) < 0 or min(room) < 0 or int(poff_host[-1]) > path.shape[0]:
            raise ValueError("poff_host must ascend within the packed path")
        path = path.to(dev, torch.int32).contiguous()
        la, lb = [int(w.numel()) for w in syn_waves], [int(w.numel()) for w in ref_waves]
        wa = torch.cat([w.to(dev, torch.float32) for w in syn_waves]).contiguous()
        wb = torch.cat([w.to(dev, torch.float32) for w in ref_waves]).contiguous()
        woffa, woffb = kk.packed_offsets(la, torch.int64, dev), kk.packed_offsets(lb, torch.int64, dev)
        aoff, boff = kk.packed_offsets(syn_frames, torch.int32, dev), kk.packed_offsets(ref_frames, torch.int32, dev)
        poff = torch.tensor([int(v) for v in poff_host], dtype=torch.int64).to(dev)
        peaks = torch.empty(2, B, dtype=torch.float32, device=dev)
        kk.call("kk_feat_peak", wa, woffa, B, max(la), peaks[0])
        kk.call("kk_feat_peak", wb, woffb, B, max(lb), peaks[1])
        sums = torch.zeros(5 * len(WINDOWS), B, dtype=torch.float64, device=dev)
        counts = torch.zeros(2, B, dtype=torch.int32, device=dev)
        tiles, toff = self.tiles(room)
        if tiles.shape[0]:
            part = torch.zeros(tiles.shape[0], 5 * len(WINDOWS), dtype=torch.float64, device=dev)
            pcnt = torch.zeros(tiles.shape[0], 2, dtype=torch.int32, device=dev)
            kk.call("kk_dtw_spectral_stats", wa, woffa, peaks[0], wb, woffb, peaks[1], aoff, boff, path, poff, steps.to(dev, torch.int32), B,
                    tiles.to(dev), tiles.shape[0], toff.to(dev), self.windows, self.tw, part, pcnt, sums, counts)
        return {"sums": sums, "counts": counts, "peaks": peaks}
