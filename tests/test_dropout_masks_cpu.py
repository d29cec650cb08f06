"""The host replica of the device counter RNG (tests/dropout_masks.py): what can be known without the kernels.  That the replica
draws the kernels' bits is what tests/test_tail_kernels_gpu.py part A checks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_masks as DM  # noqa: E402


def test_thr16_edges():
    idx = np.arange(4096)
    assert DM.threshold(0.0) == 0 and DM.threshold(-1.0) == 0 and bool(DM.keep(7, 3, idx, 0.0).all()), "p = 0: nothing is dropped"
    t = DM.threshold(1e-6)
    assert t != 0 and DM.thr16(t) == 0 and bool(DM.keep(7, 3, idx, 1e-6).all()), "p = 1e-6 rounds to a 16-bit threshold of 0"
    assert DM.threshold(0.5) == 0x80000000 and DM.thr16(DM.threshold(0.5)) == 0x8000
    assert DM.thr16(DM.threshold(0.99999)) == 0xFFFF
    assert DM.threshold(1.0) == 0xFFFFFFFF and DM.thr16(0xFFFFFFFF) == 0xFFFF and DM.thr16(0xFFFF7FFF) == 0xFFFF
    assert DM.thr16(0xFFFF8000) == 0xFFFF, "no wrap to 0 where thr + 0x8000 passes 2^32"
    assert DM.threshold(0.2) == int(float(np.float32(0.2)) * 2 ** 32) == 858993472, "the rate is the fp32 number the kernel receives"
    assert DM.thr16(DM.threshold(0.2)) == 13107


def test_pair_halves():
    """Elements 2k and 2k+1 use the low and the high half of ONE hash."""
    k = np.arange(0, 5000, dtype=np.uint64)
    h0, h1 = DM.pair_hash(77, 40, 2 * k), DM.pair_hash(77, 40, 2 * k + 1)
    assert np.array_equal(h0, h1)
    assert int(h0.max()) <= 0xFFFFFFFF and len(np.unique(h0)) > 4990, "32-bit values, no collapse"
    t = np.uint64(DM.thr16(DM.threshold(0.2)))
    assert np.array_equal(DM.keep(77, 40, 2 * k, 0.2), (h0 & np.uint64(0xFFFF)) >= t)
    assert np.array_equal(DM.keep(77, 40, 2 * k + 1, 0.2), (h0 >> np.uint64(16)) >= t)
    assert not np.array_equal(DM.keep(77, 40, 2 * k, 0.2), DM.keep(77, 40, 2 * k + 1, 0.2))
    assert not np.array_equal(DM.pair_hash(77, 40, 2 * k), DM.pair_hash(77, 41, 2 * k)), "another site, another stream"
    assert not np.array_equal(DM.pair_hash(77, 40, 2 * k), DM.pair_hash(78, 40, 2 * k)), "another seed, another stream"
    # idx >> 1 is truncated to 32 bits: the stream repeats after 2^33 elements
    assert np.array_equal(DM.pair_hash(77, 40, 2 * k), DM.pair_hash(77, 40, 2 * k + np.uint64(1 << 33)))


def test_pair_hash_one_value_by_hand():
    """kk_pair_hash(seed 1, site 2, idx 6) restated with Python integers."""
    x = (6 >> 1) ^ ((1 * 0x9E3779B9 + 2 * 0x85EBCA6B) & 0xFFFFFFFF)
    x ^= x >> 16
    x = ((x & 0xFFFFFF) * 0xb5352d) & 0xFFFFFFFF
    x ^= x >> 13
    x = ((x & 0xFFFFFF) * 0xca68b5) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(DM.pair_hash(1, 2, 6)) == x
    y = 6 ^ ((1 * 0x9E3779B9 + 2 * 0x85EBCA6B + 5 * 0xC2B2AE35) & 0xFFFFFFFF)
    y ^= y >> 16
    y = (y * 0x7feb352d) & 0xFFFFFFFF
    y ^= y >> 15
    y = (y * 0x846ca68b) & 0xFFFFFFFF
    y ^= y >> 16
    y ^= 1
    y = (y * 0x9E3779B1) & 0xFFFFFFFF
    y ^= y >> 15
    assert int(DM.hash32(1, 2, (5 << 32) + 6)) == y, "kk_hash with its idx >> 32 term"
    assert int(DM.hash32(1, 2, 6)) != y


def test_keep_scalar_equals_array():
    idx = np.arange(3000)
    for p in (0.0, 0.1, 0.25, 0.5):
        arr = DM.keep(1234, 5, idx, p)
        assert arr.dtype == bool and arr.shape == idx.shape
        assert all(bool(DM.keep(1234, 5, int(i), p)) == bool(arr[i]) for i in (0, 1, 2, 3, 999, 1000, 2999))
    rate = float(DM.keep(1234, 5, np.arange(200000), 0.2).mean())
    assert abs(rate - 0.8) < 0.005, rate


def test_tail_mask():
    ones = DM.tail_mask(77, 37, 64, 5, 40, 0.0, 41, 0.0, 42, 0.0)
    assert ones.dtype == np.float64 and ones.shape == (37, 64) and bool((ones == 1.0).all()), "all p = 0: all ones"
    m = DM.tail_mask(77, 37, 64, 5, 40, 0.2, 41, 0.1, 42, 0.25)
    k1, k2, kd = DM.tail_keeps(77, 37, 64, 5, 40, 0.2, 41, 0.1, 42, 0.25)
    assert kd.shape == (37,) and all(len(set(kd[s:s + 5].tolist())) == 1 for s in range(0, 37, 5)), "DropPath is per sample of S rows"
    assert np.array_equal(kd[::5], DM.keep(77, 42, np.arange(8), 0.25)), "sample index row // S, the last sample partial"
    assert np.array_equal(m != 0, k1 & k2 & kd[:, None])
    full = DM.inv_keep64(0.2) * DM.inv_keep64(0.1) * DM.inv_keep64(0.25)
    assert np.allclose(m[m != 0], full, rtol=1e-15)
    assert np.array_equal(k1.reshape(-1), DM.keep(77, 40, np.arange(37 * 64), 0.2)), "element index row * H + col"
    m32 = DM.tail_mask(77, 37, 64, 5, 40, 0.2, 41, 0.0, 42, 0.0, fp32_factors=True)
    assert set(np.unique(m32).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.2)))}


def test_specaug_zero_spans():
    z = DM.specaug_zero(3, 20, 16, 100, 128, 5, 3, 1, 2)
    assert z.shape == (16, 100, 128) and z.dtype == bool and z.any() and not z.all()
    for b in range(16):
        frames = z[b].all(1)
        assert int(frames.sum()) < 5, "one time mask of fewer than min(5, T // 4) frames"
        idx = np.flatnonzero(frames)
        assert len(idx) == 0 or idx[-1] - idx[0] == len(idx) - 1
        assert int(z[b][~frames].all(0).sum()) <= 4, "two feature masks of fewer than 3 dims"
    assert not DM.specaug_zero(3, 20, 4, 3, 12, 20, 5, 2, 2).all(2).any(), "T = 3: time limit 1, lengths 0, no time mask"
