"""The fp64 oracle of csrc/kk_dtw.hip: mel cepstra, dynamic time warping and the sums along a path, on the CPU in numpy.

Written from the definitions (DESIGN §5 "Alignment and free-running evaluation"):
    c_k(t)  = sqrt(2 / M) sum_m x_t[m] cos(pi k (m + 0.5) / M),  k = 1..K          the orthonormal DCT-II without its 0th coefficient
    d(i, j) = sqrt(sum_k (ca_k[i] - cb_k[j])^2)
    D(0, 0) = d(0, 0),  D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1))    steps (1,1), (1,0), (0,1), unit weights, no band
with the kernel's tie-break: the diagonal first, then (i-1, j), then (i, j-1), a later one only when strictly smaller.  The DP is
vectorised along anti-diagonals, the cells of which are independent.  Cepstra are [T, K] here ([K][T] on the device).
track_stats / track_metrics: the sums of two scalar tracks per side (normalised pitch, energy) along a path and the record fields made
of them: voicing counts, gross pitch errors, the F0 difference in cents, the energy difference.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def dct_table(M: int, K: int) -> np.ndarray:
    """[K, M] fp64: sqrt(2 / M) cos(pi k (m + 0.5) / M), k = 1..K."""
    if not (1 <= K <= 32):
        raise ValueError(f"K must be in 1..32, not {K}")
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / M) * np.cos(math.pi * k * (m + 0.5) / M)


def mcep(mel, K: int = 13) -> np.ndarray:
    """Cepstra [T, K] (fp64) of a log-mel [T, M]."""
    x = _f64(mel)
    return x @ dct_table(x.shape[1], K).T


def local_distance(ca, cb) -> np.ndarray:
    """d [Ta, Tb] of cepstra [Ta, K] and [Tb, K]."""
    ca, cb = _f64(ca), _f64(cb)
    acc = np.zeros((ca.shape[0], cb.shape[0]))
    for k in range(ca.shape[1]):
        acc += (ca[:, k, None] - cb[None, :, k]) ** 2
    return np.sqrt(acc)


def dtw(ca, cb) -> Tuple[float, np.ndarray, np.ndarray]:
    """(total = D(Ta-1, Tb-1), path int32 [steps, 2] from (0, 0) to (Ta-1, Tb-1), D [Ta, Tb])."""
    d = local_distance(ca, cb)
    Ta, Tb = d.shape
    if Ta < 1 or Tb < 1:
        raise ValueError("dtw needs at least one frame on each side")
    # the cells in diagonal order, so that a diagonal is a slice: cell n of diagonal s is (lo_s + n, s - lo_s - n)
    lo = [max(0, s - Tb + 1) for s in range(Ta + Tb - 1)]
    hi = [min(s, Ta - 1) for s in range(Ta + Tb - 1)]
    I = np.concatenate([np.arange(lo[s], hi[s] + 1) for s in range(Ta + Tb - 1)])
    J = np.repeat(np.arange(Ta + Tb - 1), [hi[s] - lo[s] + 1 for s in range(Ta + Tb - 1)]) - I
    off = np.concatenate([[0], np.cumsum([hi[s] - lo[s] + 1 for s in range(Ta + Tb - 1)])])
    dflat, Dflat, cflat = d[I, J], np.empty(I.shape), np.zeros(I.shape, dtype=np.int8)
    # p1[i + 1] = D(i, s - 1 - i), p2[i + 1] = D(i, s - 2 - i); inf wherever that cell does not exist
    p2, p1 = np.full(Ta + 1, np.inf), np.full(Ta + 1, np.inf)
    p1[1] = Dflat[0] = d[0, 0]
    for s in range(1, Ta + Tb - 1):
        a, b = lo[s], hi[s] + 1
        best, up, left = p2[a:b], p1[a:b], p1[a + 1:b + 1]          # (i-1, j-1), (i-1, j), (i, j-1) of the cells i = a .. b - 1
        c = np.zeros(b - a, dtype=np.int8)
        take = up < best                                           # a later predecessor only when strictly smaller
        best, c = np.where(take, up, best), np.where(take, np.int8(1), c)
        take = left < best
        best, c = np.where(take, left, best), np.where(take, np.int8(2), c)
        cur = np.full(Ta + 1, np.inf)
        cur[a + 1:b + 1] = Dflat[off[s]:off[s + 1]] = dflat[off[s]:off[s + 1]] + best
        cflat[off[s]:off[s + 1]] = c
        p2, p1 = p1, cur
    D, code = np.empty((Ta, Tb)), np.zeros((Ta, Tb), dtype=np.int8)
    D[I, J], code[I, J] = Dflat, cflat
    i, j = Ta - 1, Tb - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        c = code[i, j]
        i, j = i - (c != 2), j - (c != 1)
        path.append((i, j))
    return float(D[Ta - 1, Tb - 1]), np.array(path[::-1], dtype=np.int32), D


def path_cost(ca, cb, path) -> float:
    """sum of d(i, j) over the path's cells."""
    ca, cb, p = _f64(ca), _f64(cb), np.asarray(path, dtype=np.int64)
    return float(np.sqrt(((ca[p[:, 0]] - cb[p[:, 1]]) ** 2).sum(1)).sum())


def path_stats(ca, cb, xa, xb, path) -> Tuple[float, float]:
    """(mcd_sum, l1_sum) along the path: sum (10 / ln 10) sqrt(2) d(i, j) on the cepstra, sum mean_m |xa_i[m] - xb_j[m]| on the
    log-mels [T, M]; divided by the path's length they are MCD-DTW in dB and the aligned mel L1."""
    xa, xb, p = _f64(xa), _f64(xb), np.asarray(path, dtype=np.int64)
    return MCD_SCALE * path_cost(ca, cb, p), float(np.abs(xa[p[:, 0]] - xb[p[:, 1]]).mean(1).sum())


F_LO, F_SPAN = 50.0, 800.0 - 50.0 + 1e-8          # features_torch.pitch_finish: p = (f - 50) / (800 - 50 + 1e-8), 0 when unvoiced
GPE_RATIO = 0.2                                   # a gross pitch error: more than 20 % off the reference's F0
TRACK_COUNTS = ("n_vv", "n_vu", "n_uv", "n_uu", "n_gpe")
TRACK_SUMS = ("cents_sum", "cents_sq_sum", "energy_l1_sum")


def track_stats(path, pa, pb, ea, eb, f_lo: float = F_LO, f_span: float = F_SPAN, gpe_ratio: float = GPE_RATIO) -> Dict[str, float]:
    """The sums of kk_dtw_track_stats for one pair, along path [steps, 2], on the normalised pitch tracks pa [Ta], pb [Tb] and the
    energy tracks ea, eb.  A frame is voiced iff p > 0, its frequency is f = f_lo + f_span p.  Returns the int counts n_vv (both
    voiced), n_vu (a voiced, b not), n_uv, n_uu, n_gpe (both voiced and |fa - fb| > gpe_ratio fb) and the fp64 sums cents_sum,
    cents_sq_sum of c = 1200 log2(fa / fb) over the steps voiced on both sides and energy_l1_sum of |ea[i] - eb[j]| over all steps."""
    p = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    pa, pb, ea, eb = _f64(pa)[p[:, 0]], _f64(pb)[p[:, 1]], _f64(ea)[p[:, 0]], _f64(eb)[p[:, 1]]
    va, vb = pa > 0.0, pb > 0.0
    vv = va & vb
    fa, fb = f_lo + f_span * pa[vv], f_lo + f_span * pb[vv]
    c = 1200.0 * np.log2(fa / fb)
    return {"n_vv": int(vv.sum()), "n_vu": int((va & ~vb).sum()), "n_uv": int((~va & vb).sum()), "n_uu": int((~va & ~vb).sum()),
            "n_gpe": int((np.abs(fa - fb) > gpe_ratio * fb).sum()), "cents_sum": float(c.sum()), "cents_sq_sum": float((c * c).sum()),
            "energy_l1_sum": float(np.abs(ea - eb).sum())}


def track_metrics(stats: Dict[str, float], steps: int) -> Dict[str, object]:
    """What a record carries of track_stats' sums over a path of `steps` cells: f0_rmse_cents = sqrt(mean c^2), f0_bias_cents =
    mean c and gpe = n_gpe / n_vv over the steps voiced on both sides (None when there is none), vuv_err = (n_vu + n_uv) / steps,
    energy_l1_dtw = mean |ea - eb|, and the counts themselves."""
    n = int(stats["n_vv"])
    out = {"f0_rmse_cents": math.sqrt(stats["cents_sq_sum"] / n) if n else None, "f0_bias_cents": stats["cents_sum"] / n if n else None,
           "gpe": int(stats["n_gpe"]) / n if n else None, "vuv_err": (int(stats["n_vu"]) + int(stats["n_uv"])) / steps,
           "energy_l1_dtw": stats["energy_l1_sum"] / steps}
    out.update({k: int(stats[k]) for k in TRACK_COUNTS})
    return out
