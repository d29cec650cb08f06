"""GPU suite: the mixture kernels of csrc/kk_align.hip (kk_align_loglik, kk_align_mix_labels, kk_align_accumulate_mix) against the
fp64 oracle (kokoro_ruslan_amd.align_torch), evaluated from the kernels' own fp32 parameters as tests/test_align_kernels_gpu.py does.

A component value l_m is kk_align_loglik's fmaf chain plus k: that file's bound tau_m = (D + 4) 2^-23 mag_m, mag_m = sum_d |a| (x - mu)^2
+ |k|.  L = mx + logf(sum_m expf(l_m - mx)) is a weighted mean of the component errors (weights exp(l_m - L) summing to 1) plus the
rounding of every exponent's argument: at most 3 max_m tau_m; expf and logf (a few ulp each on values in [0, 1] and [0, ln M]), the
M-term sum and the last addition add (2 M + 8) 2^-23 max(1, |L|).

The labels are pinned by score, not by identity: fp32 and fp64 may rank two near components differently, but the fp64 value of the
component the kernel chose cannot lie below the fp64 maximum by more than both components' tau, written 2 tau with tau the largest of
the class at that frame."""
import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
MEL = 80


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import align as A
    from kokoro_ruslan_amd import lib as kk
    assert A.mix_frames() == 256
    return A, kk


def _model(g, c, m, d, spread=1.0):
    w = torch.rand(c, m, generator=g, dtype=torch.float64) + 0.1
    out = {"mean": torch.randn(c * m, d, generator=g, dtype=torch.float64) * spread, "var": torch.rand(c * m, d, generator=g, dtype=torch.float64) * 1.5 + 0.5}
    if m > 1:
        out.update(weight=w / w.sum(1, keepdim=True), mixtures=m)
    return out


def _host(al, model):
    """The kernel's own fp32 parameters, in fp64 on the host."""
    return tuple(t.cpu().numpy().astype(np.float64) for t in al.params(model))


def _mags(x, a, mu, k):
    """mag [G, T] of features x [T, D]."""
    return np.stack([(np.abs(a[g]) * (x - mu[g]) ** 2).sum(1) + abs(k[g]) for g in range(a.shape[0])])


def _check_loglik(L, x, a, mu, k, M, D, what):
    ref = R.loglik_mix_from_params(x, a, mu, k, M)
    fin = np.isfinite(k)
    mag = np.where(fin[:, None], _mags(x, a, mu, np.where(fin, k, 0.0)), 0.0)      # (a dropped component has no error)
    tau = (D + 4) * EPS * mag.reshape(-1, M, x.shape[0]).max(1)
    bound = 3 * tau + (2 * M + 8) * EPS * np.maximum(1.0, np.abs(ref))
    ratio = float((np.abs(L - ref) / bound).max())
    print(f"{what}: log-likelihoods, max error / bound {ratio:.3e}")
    assert L.shape == ref.shape and np.isfinite(L).all() and ratio <= 1.0
    return ref


@pytest.mark.parametrize("c,m,d", [(2, 2, 2), (118, 2, 28), (256, 4, 64)])
def test_loglik_mix_against_the_fp64_oracle(gpu, c, m, d):
    A, kk = gpu
    g = torch.Generator().manual_seed(1000 * c + d)
    states = 1 if c == 2 else 2
    al = A.PhoneAligner(K=d // 2 - 1, n_classes=c // states, states=states, mixtures=m)
    assert al.classes == c and al.gaussians == c * m
    mels = [torch.randn(T, MEL, generator=g) * 2.0 - 5.0 for T in (100, 31)]       # 131 frames: one partial workgroup, two utterances
    feat = al.features(mels)
    x = feat.cpu().numpy().astype(np.float64).T
    model = dict(_model(g, c, m, d, spread=float(np.abs(x).std())), **({"states": states} if states > 1 else {}))
    L = al.loglik(feat, model)
    assert kk.last_kernel() == "align_loglik" and L.dtype == torch.float32
    a, mu, k = _host(al, model)
    _check_loglik(L.cpu().numpy().astype(np.float64), x, a, mu, k, m, d, f"C {c} M {m} D {d}")
    # a frame's L does not depend on the batch
    alone = al.loglik(al.features(mels[1:]), model)
    assert torch.equal(alone.cpu().view(torch.int32), L[:, 100:].cpu().contiguous().view(torch.int32))
    # two components of equal weight at the same place are the single Gaussian, up to the bound's second term
    if m == 2:
        one = {"mean": model["mean"][0::2], "var": model["var"][0::2]}
        twin = {"mean": one["mean"].repeat_interleave(2, 0), "var": one["var"].repeat_interleave(2, 0), "weight": torch.full((c, 2), 0.5, dtype=torch.float64),
                "mixtures": 2, **({"states": states} if states > 1 else {})}
        single = A.PhoneAligner(K=d // 2 - 1, n_classes=c // states, states=states)
        L1 = single.loglik(feat, dict(one, **({"states": states} if states > 1 else {}))).cpu().double()
        L2 = al.loglik(feat, twin).cpu().double()
        assert float(((L2 - L1).abs() / (12 * EPS * L1.abs().clamp(min=1.0))).max()) <= 1.0


def test_a_component_with_k_of_minus_infinity_is_dropped(gpu):
    A, kk = gpu
    g = torch.Generator().manual_seed(2)
    c, m, d, T = 5, 4, 10, 77
    al = A.PhoneAligner(K=d // 2 - 1, n_classes=c, mixtures=m)
    model = _model(g, c, m, d)
    model["weight"] = torch.tensor([[0.0, 1.0, 0.0, 0.0], [0.5, 0.0, 0.5, 0.0], [0.25] * 4, [0.0, 0.0, 0.0, 1.0], [0.1, 0.2, 0.3, 0.4]], dtype=torch.float64)
    feat = (torch.randn(d, T, generator=g) * 1.5).cuda().contiguous()
    a, mu, k = _host(al, model)
    assert np.isneginf(k).sum() == 8
    L = al.loglik(feat, model).cpu().numpy().astype(np.float64)
    x = feat.cpu().numpy().astype(np.float64).T
    ref = _check_loglik(L, x, a, mu, k, m, d, "k = -inf")
    # a class with one live component is that component: no exp, no log in the way beyond expf(0) = 1 and logf(1) = 0
    comp = R.mix_components(x, a, mu, np.where(np.isfinite(k), k, 0.0))
    assert np.abs(ref[0] - comp[1]).max() == 0.0 and np.abs(ref[3] - comp[15]).max() == 0.0
    # and the labels never choose a dropped component
    lab = torch.randint(0, c, (T,), generator=g, dtype=torch.int32).cuda()
    chosen = al.mix_labels(feat, model, lab).cpu().numpy()
    assert np.isfinite(k[chosen]).all() and np.array_equal(chosen // m, lab.cpu().numpy())


@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("c,m,d", [(118, 2, 28), (59, 4, 64), (3, 2, 2)])
def test_mix_labels_choose_a_component_that_scores_the_maximum(gpu, c, m, d, T):
    A, kk = gpu
    g = torch.Generator().manual_seed(100 * c + T)
    al = A.PhoneAligner(K=d // 2 - 1, n_classes=c, mixtures=m)
    model = _model(g, c, m, d)
    feat = (torch.randn(d, T, generator=g) * 1.5).cuda().contiguous()
    lab = torch.randint(0, c, (T,), generator=g, dtype=torch.int32)
    if T > 1:
        lab[T // 3] = -1
        lab[T - 1] = c - 1
    got = al.mix_labels(feat, model, lab.cuda())
    assert kk.last_kernel() == "align_mix_labels" and got.dtype == torch.int32 and got.shape == (T,)
    got, lab = got.cpu().numpy(), lab.numpy()
    assert np.array_equal(got[lab < 0], np.full(int((lab < 0).sum()), -1))
    ok = lab >= 0
    assert np.array_equal(got[ok] // m, lab[ok]), "the component belongs to the frame's class"
    a, mu, k = _host(al, model)
    x = feat.cpu().numpy().astype(np.float64).T
    comp, mag = R.mix_components(x, a, mu, k), _mags(x, a, mu, k)
    t = np.arange(T)[ok]
    own = comp.reshape(c, m, T)[lab[ok], :, t]                                   # [frames, M]
    tau = (d + 4) * EPS * mag.reshape(c, m, T)[lab[ok], :, t].max(1)
    short = own.max(1) - comp[got[ok], t]
    print(f"C {c} M {m} D {d} T {T}: largest (maximum - chosen) / 2 tau {float((short / (2 * tau)).max()):.3e}, "
          f"{int((got[ok] != R.mix_labels_from_params(x, lab, a, mu, k, m)[ok]).sum())} of {int(ok.sum())} differ from the fp64 choice")
    assert (short <= 2 * tau).all()


def test_mix_labels_on_a_constructed_case_are_the_oracles(gpu):
    A, kk = gpu
    g = torch.Generator().manual_seed(6)
    c, m, d = 6, 4, 8
    al = A.PhoneAligner(K=d // 2 - 1, n_classes=c, mixtures=m)
    centre = torch.randn(c, 1, d, generator=g, dtype=torch.float64).float().double()
    mean = (centre + 10.0 * torch.arange(m, dtype=torch.float64)[None, :, None]).reshape(c * m, d)      # 10 sigma apart, fp32 values
    mean[4 * 2 + 1] = mean[4 * 2 + 0]                                                                   # class 2: components 0 and 1 identical
    model = {"mean": mean, "var": torch.ones(c * m, d, dtype=torch.float64), "weight": torch.full((c, m), 0.25, dtype=torch.float64), "mixtures": m}
    lens = (40, 300, 25)                                                     # the second utterance has no alignment: all labels -1
    want = torch.randint(0, c * m, (sum(lens),), generator=g)
    want[:5] = torch.tensor([8, 9, 8, 9, 10])
    feat = mean[want].float().t().contiguous().cuda()                         # frames drawn at the means
    lab = (want // m).to(torch.int32)
    lab[40:340] = -1
    got = al.mix_labels(feat, model, lab.cuda()).cpu().numpy()
    a, mu, k = _host(al, model)
    ref = R.mix_labels_from_params(feat.cpu().numpy().astype(np.float64).T, lab.numpy(), a, mu, k, m)
    assert np.array_equal(got, ref)
    assert (got[40:340] == -1).all()
    expect = want.numpy().copy()
    expect[expect == 9] = 8                                                  # the twin of component 8: the lower index wins the tie
    expect[40:340] = -1
    assert np.array_equal(got, expect) and (got[:5] == [8, 8, 8, 8, 10]).all()


def _labels(g, G, T):
    lab = torch.randint(0, G, (T,), generator=g)
    if G > 2:
        lab[lab == 1] = 0                                                    # Gaussian 1 is empty
        if T > 3:
            lab[lab == G - 1] = G - 2                                        # so is the last one ...
            lab[T // 2] = G - 1                                              # ... but for exactly one frame
    if T > 10:
        lab[3:9] = -1                                                        # frames of an infeasible utterance count nowhere
        lab[T - 1] = G + 5 if G < 1024 else -1                               # a label past the model counts nowhere either
    return lab.to(torch.int32)


@pytest.mark.parametrize("D", [2, 28, 64])
@pytest.mark.parametrize("G", [2, 300, 1024])
def test_accumulate_mix_counts_exactly_sums_in_fp64_and_repeats_bitwise(gpu, G, D):
    A, kk = gpu
    al = A.PhoneAligner(K=D // 2 - 1, n_classes=1)
    for T in (1, 255, 256, 257, 5000):
        g = torch.Generator().manual_seed(G + D + T)
        feat = (torch.randn(D, T, generator=g) * 3.0 + 1.0).cuda().contiguous()
        lab = _labels(g, G, T)
        dev = lab.cuda()
        n, s1, s2 = al.accumulate_mix(feat, dev, G)
        assert kk.last_kernel() == "align_accumulate_mix"
        n2, t1, t2 = al.accumulate_mix(feat, dev, G)
        for x, y in ((n, n2), (s1, t1), (s2, t2)):
            assert torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8)), "two runs must give the same bits"
        x = feat.cpu().numpy().astype(np.float64).T
        l = lab.numpy().astype(np.int64)
        l = np.where(l >= G, -1, l)
        rn, r1, r2 = R.accumulate([x], [l], G)
        assert n.dtype == torch.int64 and np.array_equal(n.cpu().numpy(), rn) and np.array_equal(rn, np.bincount(l[l >= 0], minlength=G))
        if G > 2 and T > 3:
            assert rn[1] == 0 and rn[G - 1] == 1
        _, m1, m2 = R.accumulate([np.abs(x)], [l], G)                          # the accumulated magnitudes (m2 = r2)
        for got, ref, mag, name in ((s1, r1, m1, "sum"), (s2, r2, m2, "sumsq")):
            got = got.cpu().numpy()
            assert got.shape == (G, D) and (np.abs(got - ref) <= 1e-12 * mag).all(), (name, G, D, T)
            assert (got[rn == 0] == 0.0).all(), "an empty Gaussian has zeros, written"
        if G <= 256:
            on, o1, o2 = (torch.empty(G, dtype=torch.int64, device="cuda"), torch.empty(G, D, dtype=torch.float64, device="cuda"),
                          torch.empty(G, D, dtype=torch.float64, device="cuda"))
            kk.call("kk_align_accumulate", feat, dev, T, D, G, on, o1, o2)
            assert torch.equal(on, n)
            assert (np.abs(o1.cpu().numpy() - s1.cpu().numpy()) <= 1e-12 * m1).all() and (np.abs(o2.cpu().numpy() - s2.cpu().numpy()) <= 1e-12 * m2).all()


def test_the_workspace_size_and_the_guards(gpu):
    A, kk = gpu
    lib = kk.load()
    assert lib.kk_align_accumulate_mix_ws_bytes(1, 2) == 4 * (2 * 1 + 2 + 1)
    assert lib.kk_align_accumulate_mix_ws_bytes(257, 1024) == 4 * (1024 * 2 + 1024 + 257)
    assert lib.kk_align_accumulate_mix_ws_bytes(2 ** 31 - 1, 1024) == 4 * (1024 * 2 ** 23 + 1024 + 2 ** 31 - 1), "64-bit arithmetic"
    assert lib.kk_align_accumulate_mix_ws_bytes(100, 1025) == 0 and lib.kk_align_accumulate_mix_ws_bytes(0, 4) == 0
    T = 40
    f = lambda d: torch.zeros(d, T, device="cuda")
    p = lambda gg, d: (torch.ones(gg, d, device="cuda") * -0.5, torch.zeros(gg, d, device="cuda"), torch.zeros(gg, device="cuda"))
    lab = torch.zeros(T, dtype=torch.int32, device="cuda")
    out = torch.zeros(T, dtype=torch.int32, device="cuda")
    kk.call("kk_align_mix_labels", f(4), T, 4, 2, 2, *p(4, 4), lab, out)      # a valid call, so that the last kernel is known
    assert kk.last_kernel() == "align_mix_labels"
    cases = [("kk_align_loglik", (f(4), T, 4, 2, 3, *p(6, 4), torch.zeros(2, T, device="cuda")), "M = 3"),
             ("kk_align_loglik", (f(4), T, 4, 2, 8, *p(16, 4), torch.zeros(2, T, device="cuda")), "M = 8"),
             ("kk_align_loglik", (f(4), T, 4, 1025, 1, *p(1025, 4), torch.zeros(1025, T, device="cuda")), "C = 1025, M = 1"),
             ("kk_align_loglik", (f(4), T, 4, 257, 4, *p(1028, 4), torch.zeros(257, T, device="cuda")), "C = 257, M = 4"),
             ("kk_align_loglik", (f(65), T, 65, 2, 2, *p(4, 65), torch.zeros(2, T, device="cuda")), "D = 65"),
             ("kk_align_mix_labels", (f(4), T, 4, 2, 3, *p(6, 4), lab, out), "M = 3"),
             ("kk_align_mix_labels", (f(4), T, 4, 2, 8, *p(16, 4), lab, out), "M = 8"),
             ("kk_align_mix_labels", (f(4), T, 4, 1025, 1, *p(1025, 4), lab, out), "C = 1025"),
             ("kk_align_mix_labels", (f(65), T, 65, 2, 2, *p(4, 65), lab, out), "D = 65")]
    for name, args, match in cases:
        with pytest.raises(RuntimeError, match=f"{name}.*{match}"):
            kk.call(name, *args)
        assert kk.last_kernel() == "align_mix_labels", "the guard stands before the launch"
    need = lib.kk_align_accumulate_mix_ws_bytes(T, 8)
    n, s = torch.zeros(1025, dtype=torch.int64, device="cuda"), torch.zeros(2, 1025, 65, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for args, match in (((f(4), lab, T, 4, 8, n, s[0], s[1], ws[:need - 1], need - 1), f"a workspace of {need - 1} bytes; needs {need}"),
                        ((f(4), lab, T, 4, 1025, n, s[0], s[1], ws, need), "G = 1025"),
                        ((f(65), lab, T, 65, 8, n, s[0], s[1], ws, need), "D = 65")):
        with pytest.raises(RuntimeError, match=f"kk_align_accumulate_mix.*{match}"):
            kk.call("kk_align_accumulate_mix", *args)
        assert kk.last_kernel() == "align_mix_labels"
    assert not n.any() and not s.any(), "nothing was written"
