"""GPU suite: kk_dtw_track_stats (csrc/kk_dtw.hip) behind MelAligner.align(tracks=) against the fp64 oracle
(kokoro_ruslan_amd.dtw_torch.track_stats) ON THE KERNEL'S OWN PATH AND THE SAME TRACKS: the voicing and gross-pitch-error counts are
equal, the three sums agree to 1e-9; bitwise batch independence; the guards.

The bound of the sums: every term is formed in fp64 on both sides from the same fp32 tracks with correctly rounded +, -, x, / and a
log2 within a few ulp, and a path has at most 8191 steps, so the sums differ by about 8191 x 4 x 2^-53 = 4e-12 relative at the most:
1e-9 relative (with an absolute floor of 1e-9 for sums near zero) leaves three orders of margin."""
import os
import sys

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import dtw_torch as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dtw_tracks_cases import close as _close, pitch_track as _pitch  # noqa: E402

pytestmark = pytest.mark.gpu

M = 80
#          1 x 1   1 x 7   self: one step per thread   one thread gets two   ragged      a never voiced   all voiced
SHAPES = [(1, 1), (1, 7), (256, 256),                  (257, 257),           (300, 257), (40, 33),        (65, 70)]
SELF, NO_A, ALL = (2, 3), 5, 6
SUMS = ("cents_sum", "cents_sq_sum", "energy_l1_sum")


def _mel(g, T):
    return torch.randn(T, M, generator=g) * 2.0 - 5.0


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.dtw import MelAligner
    g = torch.Generator().manual_seed(23)
    syn = [_mel(g, a) for a, _ in SHAPES]
    ref = [syn[n].clone() if n in SELF else _mel(g, b) for n, (_, b) in enumerate(SHAPES)]
    # side a carries one entry more than the mel has frames on every other pair (the vocoded audio's T + 1): it is cut
    pa = [_pitch(g, a + n % 2) for n, (a, _) in enumerate(SHAPES)]
    pb = [_pitch(g, b) for _, b in SHAPES]
    pa[NO_A] = torch.zeros_like(pa[NO_A])
    pa[ALL], pb[ALL] = _pitch(g, pa[ALL].numel(), 0.0), _pitch(g, pb[ALL].numel(), 0.0)
    ea = [torch.rand(a + n % 2, generator=g) for n, (a, _) in enumerate(SHAPES)]
    eb = [torch.rand(b, generator=g) for _, b in SHAPES]
    tracks = {"pitch": (pa, pb), "energy": (ea, eb)}
    al = MelAligner()
    run = al.run_packed(syn, ref, tracks)                  # one launch of each kernel for all pairs; read once, never changed
    torch.cuda.synchronize()
    host = {k: run[k].cpu().numpy() for k in ("steps", "path", "track_counts", "track_sums")}
    oracle = []
    for n, (a, b) in enumerate(SHAPES):
        p0, steps = run["poff_host"][n], int(host["steps"][n])
        path = host["path"][p0:p0 + steps]
        oracle.append((path, R.track_stats(path, pa[n][:a], pb[n], ea[n][:a], eb[n])))
    return dict(al=al, syn=syn, ref=ref, tracks=tracks, run=run, host=host, oracle=oracle)


def _sub(tracks, idx):
    return {k: tuple([side[i] for i in idx] for side in tracks[k]) for k in ("pitch", "energy")}


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_counts_equal_and_sums_agree_with_the_oracle_on_the_kernels_path(world, n):
    a, b = SHAPES[n]
    path, want = world["oracle"][n]
    counts, sums = world["host"]["track_counts"][:, n], world["host"]["track_sums"][:, n]
    print(f"pair {a} x {b}: {len(path)} steps  counts {counts.tolist()} / {[want[k] for k in R.TRACK_COUNTS]}  " +
          "  ".join(f"{k} {float(s)!r} / {want[k]!r}" for k, s in zip(SUMS, sums)))
    assert counts.dtype == np.int32 and sums.dtype == np.float64
    if n in SELF:
        assert len(path) == a and path.tolist() == [[i, i] for i in range(a)]
    assert counts.tolist() == [want[k] for k in R.TRACK_COUNTS]
    assert int(counts[:4].sum()) == len(path)
    for k, s in zip(SUMS, sums):
        assert _close(float(s), want[k]), k
    if n == NO_A:
        assert counts[0] == 0 and counts[1] == 0 and counts[4] == 0 and sums[0] == 0.0 and sums[1] == 0.0 and counts[2] > 0
    if n == ALL:
        assert counts[0] == len(path) and counts[4] > 0
    if n in (2, 3, 4):
        assert min(counts[:4]) > 0, "every voicing combination occurs"


def test_records_carry_the_metrics_of_the_kernels_sums(world):
    recs = world["al"].align(world["syn"], world["ref"], tracks=world["tracks"])
    for n, rec in enumerate(recs):
        path, want = world["oracle"][n]
        m = R.track_metrics(want, len(path))
        assert rec["steps"] == len(path) and {k: rec[k] for k in R.TRACK_COUNTS} == {k: m[k] for k in R.TRACK_COUNTS}
        assert rec["vuv_err"] == m["vuv_err"] and (rec["gpe"] == m["gpe"])
        assert _close(rec["energy_l1_dtw"] * len(path), want["energy_l1_sum"])
        if m["n_vv"]:
            assert _close(rec["f0_bias_cents"] * m["n_vv"], want["cents_sum"]) and _close(rec["f0_rmse_cents"] ** 2 * m["n_vv"], want["cents_sq_sum"])
        else:
            assert rec["f0_rmse_cents"] is None and rec["f0_bias_cents"] is None and rec["gpe"] is None
    assert recs[NO_A]["n_vv"] == 0 and recs[NO_A]["gpe"] is None
    # the mel side of the records is what align() gives without tracks
    plain = world["al"].align(world["syn"], world["ref"])
    assert [{k: r[k] for k in p} for r, p in zip(recs, plain)] == plain and "f0_rmse_cents" not in plain[0]


def test_a_pairs_track_outputs_do_not_depend_on_the_batch(world):
    al, syn, ref, tracks, batch = world["al"], world["syn"], world["ref"], world["tracks"], world["run"]
    N = len(SHAPES)
    order = list(range(N))[::-1]
    rev = al.run_packed([syn[i] for i in order], [ref[i] for i in order], _sub(tracks, order))
    for n in range(N):
        alone = al.run_packed([syn[n]], [ref[n]], _sub(tracks, [n]))
        for name in ("track_counts", "track_sums"):
            assert torch.equal(alone[name][:, 0], batch[name][:, n]), f"pair {n}: {name} differs in the batch"
            assert torch.equal(alone[name][:, 0], rev[name][:, N - 1 - n]), f"pair {n}: {name} differs in the reversed batch"


def test_groups_bounded_by_max_cells_give_the_same_records(world):
    from kokoro_ruslan_amd.dtw import dir_words
    al, syn, ref, tracks = world["al"], world["syn"], world["ref"], world["tracks"]
    one = al.align(syn, ref, tracks=tracks)
    many = al.align(syn, ref, tracks=tracks, max_cells=16 * dir_words(300, 257))            # the largest pair alone: several groups
    assert one == many and len(one) == len(SHAPES) and all("n_vv" in r for r in one)


def test_track_guards_raise_before_any_launch(world):
    from kokoro_ruslan_amd import lib as kk
    al = world["al"]
    m, t = (lambda n: torch.zeros(n, M)), (lambda n: torch.zeros(n))
    tr = lambda pa, pb, ea, eb: {"pitch": ([pa], [pb]), "energy": ([ea], [eb])}
    before = kk.launches
    with pytest.raises(ValueError, match="the synthesized pitch track has 4 entries for 5 frames"):
        al.align([m(5)], [m(3)], tracks=tr(t(4), t(3), t(5), t(3)))
    with pytest.raises(ValueError, match="the reference energy track has 4 entries for 3 frames"):
        al.align([m(5)], [m(3)], tracks=tr(t(5), t(3), t(6), t(4)))
    with pytest.raises(ValueError, match="the reference pitch track has 2 entries for 3 frames"):
        al.align([m(5)], [m(3)], tracks=tr(t(5), t(2), t(5), t(3)))
    with pytest.raises(ValueError, match="1-D float tensor"):
        al.align([m(5)], [m(3)], tracks=tr(t(5).to(torch.int32), t(3), t(5), t(3)))
    with pytest.raises(ValueError, match="1-D float tensor"):
        al.align([m(5)], [m(3)], tracks=tr(t(5), t(3), t(5)[None], t(3)))
    with pytest.raises(ValueError, match="tracks must be"):
        al.align([m(5)], [m(3)], tracks={"pitch": ([t(5)], [t(3)])})
    assert kk.launches == before
