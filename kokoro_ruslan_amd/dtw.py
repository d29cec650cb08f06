"""Dynamic time warping of mel pairs on the device, on the kernels of csrc/kk_dtw.hip: the alignment behind MCD-DTW.

A synthesized mel and its ground truth differ in length, so a frame-wise distance needs an alignment first.  `MelAligner.align` takes
the pairs of a whole validation split: it packs them back to back, projects the log-mels to K cepstra (the DCT-II without c0), runs the
DP of every pair of a group in one launch (one workgroup per pair), walks the paths back and sums the distances along them.  A pair's
results are, bit for bit, what it gives alone.  dtw_torch is the fp64 oracle of every step.

With `tracks` (the pitch and energy tracks of both sides: of the vocoded audio and of the ground truth) one more launch walks the same
paths and sums the track errors along them: the F0 error in cents over the steps voiced on both sides, the voicing decision error,
the gross pitch errors and the energy error (kk_dtw_track_stats).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.dtw_torch import F_LO, F_SPAN, GPE_RATIO, TRACK_COUNTS, TRACK_SUMS, dct_table, track_metrics

MAX_FRAMES = 4096                        # the longest side the DP kernel takes (the positional table's order)
MAX_MEL = 128                            # kk_mcep stages 64 frames of at most this many channels
DEFAULT_MAX_CELLS = 1 << 28              # cells of a group's direction buffer (2 bits each: 64 MiB)


def dir_words(Ta: int, Tb: int) -> int:
    """32-bit direction words of a Ta x Tb pair: 16 cells of a row per word."""
    return Ta * ((Tb + 15) // 16)


def _check_pair(i: int, s: torch.Tensor, r: torch.Tensor) -> None:
    for what, x in (("synthesized", s), ("reference", r)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
            raise ValueError(f"pair {i}: the {what} mel must be a float tensor [frames, mels]")
        if x.shape[0] < 1:
            raise ValueError(f"pair {i}: the {what} mel is empty")
        if x.shape[0] > MAX_FRAMES:
            raise ValueError(f"pair {i}: the {what} mel has {x.shape[0]} frames; at most {MAX_FRAMES}")
    if s.shape[1] != r.shape[1]:
        raise ValueError(f"pair {i}: {s.shape[1]} synthesized mel channels against {r.shape[1]}")


def _check_tracks(tracks, syn: Sequence[torch.Tensor], ref: Sequence[torch.Tensor]) -> None:
    if not isinstance(tracks, dict) or set(tracks) != {"pitch", "energy"}:
        raise ValueError('tracks must be {"pitch": (side a, side b), "energy": (side a, side b)}')
    for name in ("pitch", "energy"):
        sides = tracks[name]
        if not isinstance(sides, (tuple, list)) or len(sides) != 2:
            raise ValueError(f"tracks[{name!r}] must be a pair (side a, side b) of lists")
        for what, side, mels in (("synthesized", sides[0], syn), ("reference", sides[1], ref)):
            if len(side) != len(mels):
                raise ValueError(f"tracks[{name!r}]: {len(side)} {what} tracks for {len(mels)} pairs")
            for i, (x, m) in enumerate(zip(side, mels)):
                if not isinstance(x, torch.Tensor) or x.dim() != 1 or not x.is_floating_point():
                    raise ValueError(f"pair {i}: the {what} {name} track must be a 1-D float tensor")
                T = int(m.shape[0])
                if what == "synthesized" and x.shape[0] < T:
                    raise ValueError(f"pair {i}: the synthesized {name} track has {x.shape[0]} entries for {T} frames")
                if what == "reference" and x.shape[0] != T:
                    raise ValueError(f"pair {i}: the reference {name} track has {x.shape[0]} entries for {T} frames")


class MelAligner:
    """Batched DTW on the MI355X: align(synthesized mels, ground-truth mels) -> one record per pair."""

    def __init__(self, device: str = "cuda", K: int = 13, gpe_ratio: float = GPE_RATIO):
        if int(K) != K or not (1 <= K <= 32):
            raise ValueError(f"K must be an integer in 1..32, not {K!r}")
        if not (isinstance(gpe_ratio, (int, float)) and math.isfinite(gpe_ratio) and gpe_ratio >= 0):
            raise ValueError(f"gpe_ratio must be a finite number >= 0, not {gpe_ratio!r}")
        self.device, self.K, self.gpe_ratio = torch.device(device), int(K), float(gpe_ratio)
        self._tables: Dict[int, torch.Tensor] = {}

    def table(self, M: int) -> torch.Tensor:
        """[K, M] fp32 on the device: sqrt(2 / M) cos(pi k (m + 0.5) / M), evaluated in fp64 and rounded once."""
        if M not in self._tables:
            self._tables[M] = torch.from_numpy(dct_table(M, self.K)).to(torch.float32).to(self.device).contiguous()
        return self._tables[M]

    def mcep(self, mel: torch.Tensor) -> torch.Tensor:
        """Cepstra [K, T] of packed fp32 log-mels [T, M] on the device."""
        T, M = mel.shape
        out = torch.empty(self.K, T, dtype=torch.float32, device=self.device)
        kk.call("kk_mcep", mel, T, M, self.K, self.table(M), out)
        return out

    def align(self, syn: Sequence[torch.Tensor], ref: Sequence[torch.Tensor], want_path: bool = False,
              max_cells: int = DEFAULT_MAX_CELLS, tracks: Optional[Dict] = None) -> List[Dict]:
        """syn, ref: lists of log-mels [T, M] on any device, pair i = (syn[i], ref[i]).  Returns per pair {"total": D(Ta-1, Tb-1),
        "steps": cells of the optimal path, "mcd_dtw": mel-cepstral distortion in dB averaged over the path, "mel_l1_dtw": mean
        |difference| of the aligned log-mels, "len_ratio": Ta / Tb} and, with want_path, "path": int32 [steps, 2] on the device.
        The pairs run in groups whose direction buffers hold at most max_cells cells; a group costs one read by the host.
        tracks = {"pitch": (list_a, list_b), "energy": (list_a, list_b)}: 1-D float tensors per pair, the normalised pitch (0 =
        unvoiced) and energy per frame.  They are taken as fp32: a track of another float dtype is rounded to fp32 before the kernel
        sees it (the cache and FeatureExtractor hold fp32), so an oracle fed the unrounded values may count differently.  Side a has
        at least syn[i].shape[0] entries and is cut to that many (audio vocoded from a T-frame mel yields T or T + 1 feature frames;
        frame i is centred on sample 256 i on both sides), side b exactly ref[i].shape[0].  Each record then also carries, along the same path, "f0_rmse_cents", "f0_bias_cents" and "gpe" (the share
        of steps voiced on both sides whose F0 is more than gpe_ratio off the reference's); all three None when no step is voiced on
        both sides; "vuv_err" (the share of steps voiced on one side only), "energy_l1_dtw" and the counts n_vv, n_vu, n_uv, n_uu,
        n_gpe (dtw_torch.track_metrics)."""
        if len(syn) != len(ref):
            raise ValueError(f"{len(syn)} synthesized mels for {len(ref)} reference mels")
        if int(max_cells) != max_cells or max_cells < 1:
            raise ValueError(f"max_cells must be an integer >= 1, not {max_cells!r}")
        for i, (s, r) in enumerate(zip(syn, ref)):
            _check_pair(i, s, r)
        if tracks is not None:
            _check_tracks(tracks, syn, ref)
        M = {int(s.shape[1]) for s in syn}
        if len(M) > 1:
            raise ValueError(f"the pairs differ in mel channels: {sorted(M)}")
        if M and max(M) > MAX_MEL:
            raise ValueError(f"{max(M)} mel channels; at most {MAX_MEL}")
        cells = [16 * dir_words(s.shape[0], r.shape[0]) for s, r in zip(syn, ref)]
        for i, c in enumerate(cells):
            if c > max_cells:
                raise ValueError(f"pair {i}: {syn[i].shape[0]} x {ref[i].shape[0]} frames need {c} direction cells; max_cells is {max_cells}")
        out: List[Dict] = [None] * len(syn)
        group, total = [], 0
        for i in list(range(len(syn))) + [None]:
            if group and (i is None or total + cells[i] > max_cells):
                if tracks is None:
                    g = self.run_packed([syn[k] for k in group], [ref[k] for k in group])
                    host = torch.stack([g["total"].double(), g["steps"].double(), g["mcd_sum"], g["l1_sum"]]).cpu().tolist()
                else:
                    g = self.run_packed([syn[k] for k in group], [ref[k] for k in group],
                                        {name: tuple([side[k] for k in group] for side in tracks[name]) for name in ("pitch", "energy")})
                    host = torch.cat([torch.stack([g["total"].double(), g["steps"].double(), g["mcd_sum"], g["l1_sum"]]),
                                      g["track_counts"].double(), g["track_sums"]]).cpu().tolist()
                for n, k in enumerate(group):
                    steps = int(host[1][n])
                    rec = {"total": host[0][n], "steps": steps, "mcd_dtw": host[2][n] / steps, "mel_l1_dtw": host[3][n] / steps,
                           "len_ratio": syn[k].shape[0] / ref[k].shape[0]}
                    if tracks is not None:
                        rec.update(track_metrics(dict(zip(TRACK_COUNTS + TRACK_SUMS, (row[n] for row in host[4:]))), steps))
                    if want_path:
                        p0 = g["poff_host"][n]
                        rec["path"] = g["path"][p0:p0 + steps]
                    out[k] = rec
                group, total = [], 0
            if i is not None:
                group.append(i)
                total += cells[i]
        return out

    def run_packed(self, syn: Sequence[torch.Tensor], ref: Sequence[torch.Tensor], tracks: Optional[Dict] = None) -> Dict:
        """One group on the device, nothing read back: the pairs packed, their cepstra, the DP, the paths and the sums along them.
        Returns the device tensors total fp32 [B], steps int32 [B], mcd_sum / l1_sum fp64 [B], path int32 [sum (Ta + Tb - 1), 2], dir
        (the direction words), ca / cb [K, T_total] and the host lists poff_host / doff_host (first path entry / direction word of
        each pair).  With tracks (as align() takes them, already checked): also track_counts int32 [5, B] (n_vv, n_vu, n_uv, n_uu,
        n_gpe) and track_sums fp64 [3, B] (sum c, sum c^2, sum |energy difference|), and the packed tracks pa, ea, pb, eb."""
        dev, B, K = self.device, len(syn), self.K
        na, nb = [int(s.shape[0]) for s in syn], [int(r.shape[0]) for r in ref]
        xa = torch.cat([s.to(dev, torch.float32) for s in syn]).contiguous()
        xb = torch.cat([r.to(dev, torch.float32) for r in ref]).contiguous()
        M = xa.shape[1]
        doff_h = kk.packed_offsets([dir_words(a, b) for a, b in zip(na, nb)])
        poff_h = kk.packed_offsets([a + b - 1 for a, b in zip(na, nb)])
        aoff, boff = kk.packed_offsets(na, torch.int32, dev), kk.packed_offsets(nb, torch.int32, dev)
        doff, poff = doff_h.to(dev), poff_h.to(dev)
        ca, cb = self.mcep(xa), self.mcep(xb)
        total = torch.zeros(B, dtype=torch.float32, device=dev)
        dirs = torch.empty(int(doff_h[-1]), dtype=torch.int32, device=dev)
        path = torch.zeros(int(poff_h[-1]), 2, dtype=torch.int32, device=dev)
        steps = torch.zeros(B, dtype=torch.int32, device=dev)
        sums = torch.zeros(2, B, dtype=torch.float64, device=dev)
        kk.call("kk_dtw", ca, ca.shape[1], cb, cb.shape[1], K, aoff, boff, doff, B, total, dirs)
        kk.call("kk_dtw_backtrack", dirs, doff, aoff, boff, poff, B, path, steps)
        kk.call("kk_dtw_path_stats", ca, ca.shape[1], cb, cb.shape[1], K, xa, xb, M, aoff, boff, path, poff, steps, B, sums[0], sums[1])
        out = {"total": total, "steps": steps, "mcd_sum": sums[0], "l1_sum": sums[1], "path": path, "dir": dirs, "ca": ca, "cb": cb,
               "poff_host": poff_h.tolist(), "doff_host": doff_h.tolist()}
        if tracks is not None:
            pack = lambda side, n: torch.cat([x[:t].to(dev, torch.float32) for x, t in zip(side, n)]).contiguous()
            pa, pb = pack(tracks["pitch"][0], na), pack(tracks["pitch"][1], nb)
            ea, eb = pack(tracks["energy"][0], na), pack(tracks["energy"][1], nb)
            counts = torch.zeros(5, B, dtype=torch.int32, device=dev)
            tsums = torch.zeros(3, B, dtype=torch.float64, device=dev)
            kk.call("kk_dtw_track_stats", pa, ea, pb, eb, aoff, boff, path, poff, steps, B, F_LO, F_SPAN, self.gpe_ratio, counts, tsums)
            out.update(track_counts=counts, track_sums=tsums, pa=pa, ea=ea, pb=pb, eb=eb)
        return out
