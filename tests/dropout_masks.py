"""Host replica of the device counter RNG (kokoro_ruslan_amd/csrc/kk_common.h: kk_hash, kk_pair_hash, kk_drop_threshold, kk_thr16,
kk_drop_mul) and of the masks that kk_dropout.hip builds from it.  Not a test: with it a test knows every mask bit of a launch from
(seed, call site, element index) alone.  numpy on uint64, every 32-bit wrap written out as `& 0xFFFFFFFF`."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)


def _u(x):
    return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


def _idx(idx):
    return np.asarray(idx).astype(np.uint64)


def _key(seed, site):
    return (((_u(seed) & M32) * _u(0x9E3779B9) & M32) + ((_u(site) & M32) * _u(0x85EBCA6B) & M32)) & M32


def pair_hash(seed, site, idx):
    """kk_pair_hash: one hash per element PAIR (idx >> 1, truncated to 32 bits); __umul24 = low 24 bits of x times the constant, low
    32 bits of the product."""
    x = ((_idx(idx) >> _u(1)) & M32) ^ _key(seed, site)
    x = x ^ (x >> _u(16))
    x = ((x & M24) * _u(0xb5352d)) & M32
    x = x ^ (x >> _u(13))
    x = ((x & M24) * _u(0xca68b5)) & M32
    return x ^ (x >> _u(16))


def hash32(seed, site, idx):
    """kk_hash: the full 32-bit hash (SpecAugment draws its spans from it), with the idx >> 32 term."""
    idx = _idx(idx)
    s = _u(seed) & M32
    x = (idx & M32) ^ ((_key(seed, site) + (((idx >> _u(32)) & M32) * _u(0xC2B2AE35) & M32)) & M32)
    x = x ^ (x >> _u(16))
    x = (x * _u(0x7feb352d)) & M32
    x = x ^ (x >> _u(15))
    x = (x * _u(0x846ca68b)) & M32
    x = x ^ (x >> _u(16))
    x = x ^ s
    x = (x * _u(0x9E3779B1)) & M32
    return x ^ (x >> _u(15))


def threshold(p):
    """kk_drop_threshold of the fp32 rate the kernel receives: drop iff hash < threshold."""
    p = float(np.float32(p))
    return 0 if p <= 0.0 else (0xFFFFFFFF if p >= 1.0 else int(p * 4294967296.0))


def thr16(thr):
    """kk_thr16: the rate quantised to 1/65536, rounded."""
    return 0xFFFF if thr >= 0xFFFF8000 else ((thr + 0x8000) & 0xFFFFFFFF) >> 16


def keep(seed, site, idx, p):
    """bool, shaped like idx: the element is kept iff its 16-bit field (low: even idx, high: odd idx) is >= thr16."""
    idx = _idx(idx)
    thr = threshold(p)
    if thr == 0:
        return np.ones(idx.shape, dtype=bool)
    h = pair_hash(seed, site, idx)
    field = np.where((idx & _u(1)) != 0, h >> _u(16), h & _u(0xFFFF))
    return field >= _u(thr16(thr))


def inv_keep32(p):
    """1.f / (1.f - p) as the kernels compute it (fp32), 1 for p <= 0."""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p > 0 else np.float32(1.0)


def inv_keep64(p):
    """1 / (1 - p) of the fp32 rate the kernel receives, in double."""
    p = float(np.float32(p))
    return 1.0 / (1.0 - p) if p > 0 else 1.0


def tail_keeps(seed, rows, H, S, site1, p1, site2, p2, site_dp, dp):
    """(keep1 [rows, H], keep2 [rows, H], keep_dp [rows]): element masks indexed by row * H + col, DropPath by sample row // S."""
    idx = np.arange(rows * H, dtype=np.uint64).reshape(rows, H)
    return keep(seed, site1, idx, p1), keep(seed, site2, idx, p2), keep(seed, site_dp, np.arange(rows, dtype=np.uint64) // _u(S), dp)


def tail_mask(seed, rows, H, S, site1, p1, site2, p2, site_dp, dp, fp32_factors=False):
    """float64 [rows, H] multiplier keep1/(1-p1) * keep2/(1-p2) * keep_dp[row // S]/(1-dp).  fp32_factors: each 1/(1-p) is the fp32
    division of the kernels (their product still exact in double), for bit-level checks."""
    k1, k2, kd = tail_keeps(seed, rows, H, S, site1, p1, site2, p2, site_dp, dp)
    inv = (lambda p: float(inv_keep32(p))) if fp32_factors else inv_keep64
    return (k1 * inv(p1)) * (k2 * inv(p2)) * (kd * inv(dp))[:, None]


def specaug_zero(seed, site, B, T, H, tmax, fmax, nt, nf):
    """bool [B, T, H]: what specaug_kernel zeroes.  Per sample b, mask k: time length hash32(64 b + 2 k) % max(1, min(tmax, T // 4))
    at hash32(64 b + 2 k + 1) % max(1, T - length); feature length hash32(64 b + 32 + 2 k) % max(1, fmax) at
    hash32(64 b + 33 + 2 k) % max(1, H - length)."""
    z = np.zeros((B, T, H), dtype=bool)
    time_limit = max(1, min(tmax, T // 4))
    for b in range(B):
        for k in range(nt):
            n = int(hash32(seed, site, b * 64 + 2 * k)) % time_limit
            t0 = int(hash32(seed, site, b * 64 + 2 * k + 1)) % max(1, T - n)
            z[b, t0:t0 + n, :] = True
        for k in range(nf):
            n = int(hash32(seed, site, b * 64 + 32 + 2 * k)) % max(1, fmax)
            f0 = int(hash32(seed, site, b * 64 + 32 + 2 * k + 1)) % max(1, H - n)
            z[b, :, f0:f0 + n] = True
    return z
