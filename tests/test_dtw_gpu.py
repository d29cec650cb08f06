"""GPU suite: the DTW kernels (csrc/kk_dtw.hip) behind MelAligner against the fp64 oracle (kokoro_ruslan_amd.dtw_torch): degenerate
lengths, direction-word and diagonal-pass edges, one pair at the workload's size, the exact zero-cost cases, the cepstral projection,
the sums along the path, bitwise batch independence and the guards.

The kernel's path is not compared cell by cell with the oracle's: fp32 near-ties may legitimately choose differently.  What pins the
recurrence is cost: with D64 the oracle's fp64 optimum ON THE KERNEL'S OWN fp32 cepstra, |total - D64| <= tol D64 and the fp64 cost of
the kernel's path <= D64 (1 + tol), tol = (Ta + Tb + 32) 2^-23: the bound of a sequential fp32 sum of Ta + Tb non-negative terms
((n - 1) 2^-24 relative, doubled) plus the rounding of a cell's distance (a 13-term fmaf chain and a square root: below 32 2^-24)."""
import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import dtw_torch as R

pytestmark = pytest.mark.gpu

M = 80
EPS = 2.0 ** -23


def _mel(g, T, m=M):
    return torch.randn(T, m, generator=g) * 2.0 - 5.0


def _warped(g, x, Tb):
    """x read at Tb monotone positions plus a little noise: a pair that has an alignment worth finding."""
    idx = torch.linspace(0, x.shape[0] - 1, Tb).round().long()
    return x[idx] + 0.1 * torch.randn(Tb, x.shape[1], generator=g)


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib as kk
    from kokoro_ruslan_amd.dtw import MelAligner
    W = int(kk.load().kk_dtw_tile())
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 15), (5, 16), (5, 17), (5, 33), (W - 1, 3), (3, W + 1), (W, W), (W + 1, W - 1),
              (1600, 1800)]
    g = torch.Generator().manual_seed(11)
    syn = [_mel(g, a) for a, _ in shapes]
    ref = [_warped(g, s, b) if min(a, b) >= W - 1 else _mel(g, b) for s, (a, b) in zip(syn, shapes)]
    al = MelAligner()
    run = al.run_packed(syn, ref)                          # one launch of each kernel for all pairs; read once, never changed
    torch.cuda.synchronize()
    host = {k: run[k].cpu().numpy() for k in ("total", "steps", "mcd_sum", "l1_sum", "path", "ca", "cb")}
    aoff = np.cumsum([0] + [a for a, _ in shapes])
    boff = np.cumsum([0] + [b for _, b in shapes])
    oracle = {}

    def pair(n):
        """Everything about pair n on the host: kernel outputs and the fp64 oracle on the kernel's fp32 cepstra."""
        if n not in oracle:
            ca, cb = host["ca"][:, aoff[n]:aoff[n + 1]].T, host["cb"][:, boff[n]:boff[n + 1]].T
            steps = int(host["steps"][n])
            p0 = run["poff_host"][n]
            D64, _, _ = R.dtw(ca, cb)
            oracle[n] = dict(ca=ca, cb=cb, steps=steps, path=host["path"][p0:p0 + steps], total=float(host["total"][n]), D64=D64,
                             mcd_sum=float(host["mcd_sum"][n]), l1_sum=float(host["l1_sum"][n]), cap=run["poff_host"][n + 1] - p0)
        return oracle[n]
    return dict(W=W, shapes=shapes, syn=syn, ref=ref, al=al, pair=pair)


N_SHAPES = 13


@pytest.mark.parametrize("n", range(N_SHAPES))
def test_path_is_valid_and_costs_the_optimum(world, n):
    Ta, Tb = world["shapes"][n]
    r = world["pair"](n)
    p = r["path"]
    assert r["cap"] == Ta + Tb - 1 and max(Ta, Tb) <= r["steps"] <= Ta + Tb - 1
    assert p.shape == (r["steps"], 2) and p[0].tolist() == [0, 0] and p[-1].tolist() == [Ta - 1, Tb - 1]
    assert set(map(tuple, np.diff(p, axis=0).tolist())) <= {(1, 1), (1, 0), (0, 1)}
    tol = (Ta + Tb + 32) * EPS
    cost = R.path_cost(r["ca"], r["cb"], p)
    print(f"pair {Ta} x {Tb}: total {r['total']!r}  D64 {r['D64']!r}  rel {abs(r['total'] - r['D64']) / r['D64']:.3e}  "
          f"path cost rel {(cost - r['D64']) / r['D64']:.3e}  tol {tol:.3e}")
    assert abs(r["total"] - r["D64"]) <= tol * r["D64"]
    assert cost <= r["D64"] * (1 + tol)


@pytest.mark.parametrize("n", range(N_SHAPES))
def test_path_stats_are_the_oracles_sums_on_the_kernels_path(world, n):
    r = world["pair"](n)
    mcd, l1 = R.path_stats(r["ca"], r["cb"], world["syn"][n], world["ref"][n], r["path"])
    tol = r["steps"] * EPS
    print(f"pair {world['shapes'][n]}: mcd_sum rel {abs(r['mcd_sum'] - mcd) / mcd:.3e}  l1_sum rel {abs(r['l1_sum'] - l1) / l1:.3e}  tol {tol:.3e}")
    assert abs(r["mcd_sum"] - mcd) <= tol * mcd
    assert abs(r["l1_sum"] - l1) <= tol * l1


@pytest.mark.parametrize("T", [1, 16, 45, 1030])
def test_self_alignment_and_frame_doubled_copy_are_exact(world, T):
    g = torch.Generator().manual_seed(T)
    x = _mel(g, T)
    same, doubled = world["al"].align([x, x], [x.clone(), x.repeat_interleave(2, dim=0)], want_path=True)
    assert same["total"] == 0.0 and same["steps"] == T and same["mcd_dtw"] == 0.0 and same["mel_l1_dtw"] == 0.0 and same["len_ratio"] == 1.0
    assert same["path"].dtype == torch.int32 and same["path"].cpu().tolist() == [[i, i] for i in range(T)]
    assert doubled["total"] == 0.0 and doubled["steps"] == 2 * T and doubled["len_ratio"] == 0.5
    assert doubled["mcd_dtw"] == 0.0 and doubled["mel_l1_dtw"] == 0.0
    assert doubled["path"].cpu().tolist() == [[j // 2, j] for j in range(2 * T)]


@pytest.mark.parametrize("m", [80, 20])
@pytest.mark.parametrize("K", [1, 13, 32])
def test_mcep_against_the_fp64_oracle(world, K, m):
    from kokoro_ruslan_amd.dtw import MelAligner
    x = _mel(torch.Generator().manual_seed(100 * K + m), 131, m)       # three workgroups, the last one partial
    got = MelAligner(K=K).mcep(x.cuda().contiguous()).cpu().numpy()
    assert got.shape == (K, 131)
    err = float(np.abs(got.T - R.mcep(x, K)).max())
    tol = m * EPS * float(x.abs().max())
    print(f"K {K} M {m}: max abs error {err:.3e}  tol {tol:.3e}")
    assert err <= tol


def _pieces(run, n):
    """Every output of pair n of a run_packed() result, as host tensors."""
    d0, d1, p0, p1 = run["doff_host"][n], run["doff_host"][n + 1], run["poff_host"][n], run["poff_host"][n + 1]
    return [run["total"][n:n + 1].cpu(), run["steps"][n:n + 1].cpu(), run["mcd_sum"][n:n + 1].cpu(), run["l1_sum"][n:n + 1].cpu(),
            run["dir"][d0:d1].cpu(), run["path"][p0:p1].cpu()]


def test_a_pairs_outputs_do_not_depend_on_the_batch(world):
    W, al = world["W"], world["al"]
    shapes = [(1, 9), (33, 47), (W + 76, 90), (17, 16), (64, 130)]
    g = torch.Generator().manual_seed(5)
    syn, ref = [_mel(g, a) for a, _ in shapes], [_mel(g, b) for _, b in shapes]
    batch = al.run_packed(syn, ref)
    rev = al.run_packed(syn[::-1], ref[::-1])
    for n in range(len(shapes)):
        alone = _pieces(al.run_packed([syn[n]], [ref[n]]), 0)
        assert int(alone[1]) >= max(shapes[n])
        for name, x, y, z in zip(("total", "steps", "mcd_sum", "l1_sum", "dir", "path"), alone, _pieces(batch, n), _pieces(rev, len(shapes) - 1 - n)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"pair {n}: {name} differs in the batch"
            assert torch.equal(x.view(torch.uint8), z.view(torch.uint8)), f"pair {n}: {name} differs in the reversed batch"


def test_groups_bounded_by_max_cells_give_the_same_records(world):
    syn, ref = world["syn"][:8], world["ref"][:8]
    one = world["al"].align(syn, ref)
    many = world["al"].align(syn, ref, max_cells=16 * 15)               # the largest of them alone: several groups
    assert one == many and len(one) == 8
    for n, rec in enumerate(one):
        r = world["pair"](n)
        assert rec["steps"] == r["steps"] and rec["total"] == r["total"] and rec["mcd_dtw"] == r["mcd_sum"] / r["steps"]
        assert rec["len_ratio"] == world["shapes"][n][0] / world["shapes"][n][1] and "path" not in rec


def test_guards_raise_before_any_launch(world):
    from kokoro_ruslan_amd import lib as kk
    al, m = world["al"], lambda t: torch.zeros(t, M)
    before = kk.launches
    with pytest.raises(ValueError, match="4097 frames"):
        al.align([m(4097)], [m(5)])
    with pytest.raises(ValueError, match="4097 frames"):
        al.align([m(5), m(5)], [m(5), m(4097)])
    with pytest.raises(ValueError, match="pair 1: the synthesized mel is empty"):
        al.align([m(5), m(0)], [m(5), m(5)])
    with pytest.raises(ValueError, match="pair 1: 40 x 17 frames"):
        al.align([m(3), m(40)], [m(3), m(17)], max_cells=1279)
    assert kk.launches == before
