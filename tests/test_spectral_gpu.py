"""GPU suite: kk_dtw_spectral_stats (kokoro_ruslan_amd.spectral.SpectralDistance) against the fp64 oracle spectral_torch on the smallest
shapes at which it can go wrong, its independence of the batch, and the new fields of evaluate() / evaluate_vocoder() on a tiny
random-weight 80-mel engine with Griffin-Lim at 2 iterations.

The cases (one batch, computed once): waveforms of 1280, 1792, 2304 samples for mels of 5, 7, 9 frames (a HiFi-GAN's 256 T), one of
exactly 1024 samples, one all zeros, one of 256 (T - 1) samples (Griffin-Lim's length: the last frame's centre equals n and is still
counted); a path with all three step kinds, paths of one tile - 1, one tile, one tile + 1 and two tiles + 1 steps (the tile is the
kernel's constant), and a path with indices out of range and frame centres beyond the end of the waveform.

Bounds: the counts are exact; sum AB, sum A^2, sum B^2 within 1e-5 relative (the bound of every fp32 FFT kernel here); sum d and
sum d^2 at most 4x as far from fp64 as the same sums from fp32 torch.stft on the same input (the margin of the log-mel check of
test_features_kernels_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import features_torch as FT
from kokoro_ruslan_amd import spectral_torch as R
from kokoro_ruslan_amd.stft import HOP, N_FFT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _sig(n, seed):
    return FT.test_signal(n, seed=seed, f0=110.0 + 15.0 * seed).float()


def _sorted_path(g, steps, Ta, Tb):
    """`steps` steps with ascending i and j over all of [0, Ta) x [0, Tb): every frame, many repeats."""
    i = torch.sort(torch.cat([torch.arange(Ta), torch.randint(0, Ta, (steps - Ta,), generator=g)])).values
    j = torch.sort(torch.cat([torch.arange(Tb), torch.randint(0, Tb, (steps - Tb,), generator=g)])).values
    return torch.stack([i, j], 1).to(torch.int32)


def _cases(tile):
    g = torch.Generator().manual_seed(11)
    w1280, w1792, w2304, w1024 = _sig(1280, 0), _sig(1792, 1), _sig(2304, 2), _sig(1024, 3)
    gl = _sig(256 * 7, 4)                                # an 8-frame mel through Griffin-Lim: frame 7 is centred on sample n
    kinds = torch.tensor([[0, 0], [1, 1], [1, 2], [2, 2], [3, 3], [3, 4], [3, 5], [4, 5], [4, 6]], dtype=torch.int32)
    bad = torch.tensor([[0, 0], [5, 1], [6, 2], [9, 0], [-1, 3], [2, 7], [2 ** 31 - 1, 1], [3, 3], [8, -(2 ** 31)], [4, 6]], dtype=torch.int32)
    return [   # (name, a, Ta, b, Tb, path, counted, skipped)
        ("three step kinds", w1280, 5, w1792, 7, kinds, 9, 0),
        ("one tile - 1", w2304, 9, w1024, 5, _sorted_path(g, tile - 1, 9, 5), tile - 1, 0),
        ("one tile, Griffin-Lim's length", gl, 8, w1280, 6, _sorted_path(g, tile, 8, 6), tile, 0),
        ("one tile + 1", w1280, 5, w1792, 7, _sorted_path(g, tile + 1, 5, 7), tile + 1, 0),
        ("two tiles + 1", w2304, 9, w1024, 5, _sorted_path(g, 2 * tile + 1, 9, 5), 2 * tile + 1, 0),
        ("a silent side", torch.zeros(1792), 7, w2304, 9, torch.arange(7, dtype=torch.int32)[:, None].repeat(1, 2), 7, 0),
        # a mel of 9 frames whose waveform ends at 1280: (5, 1) is centred on n and counted, (6, 2) lies beyond it; the others are
        # indices outside [0, 9) x [0, 7)
        ("bad steps", w1280, 9, w1792, 7, bad, 4, 6),
    ]


def _run(sd, cases):
    """(sums fp64 [15, B], counts int32 [2, B]) on the host, through run_packed."""
    from kokoro_ruslan_amd import lib as kk
    n = [int(c[5].shape[0]) for c in cases]
    g = sd.run_packed([c[1] for c in cases], [c[3] for c in cases], torch.cat([c[5] for c in cases]).cuda(), kk.packed_offsets(n).tolist(),
                      torch.tensor(n, dtype=torch.int32).cuda(), [c[2] for c in cases], [c[4] for c in cases])
    assert g["sums"].is_cuda and g["counts"].is_cuda
    return g["sums"].cpu(), g["counts"].cpu()


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.spectral import SpectralDistance
    sd = SpectralDistance()
    cases = _cases(sd.tile)
    sums, counts = _run(sd, cases)                       # computed once, never changed
    want = [R.spectral_stats(c[1], c[3], c[5], c[2], c[4]) for c in cases]
    return dict(sd=sd, cases=cases, sums=sums, counts=counts, want=want)


def _torch32_sums(a, b, path, Ta, Tb):
    """sum d and sum d^2 per window from fp32 torch.stft on the same fp32 input, the sums themselves in fp64 as the kernel forms them."""
    a, b = FT.normalise(a, torch.float32), FT.normalise(b, torch.float32)
    path = path.long()
    i, j = path[:, 0], path[:, 1]
    ok = (i >= 0) & (i < Ta) & (j >= 0) & (j < Tb) & (HOP * i <= a.numel()) & (HOP * j <= b.numel())
    out = []
    for w in R.WINDOWS:
        win = torch.hann_window(w, periodic=True, dtype=torch.float64).float()
        PA, PB = ((lambda X: (X.real ** 2 + X.imag ** 2).double())(torch.stft(x, N_FFT, HOP, w, win, center=True, pad_mode="reflect",
                                                                          onesided=True, return_complex=True)) for x in (a, b))
        d = 10.0 * torch.log10((PA[:, i[ok]] + 1e-9) / (PB[:, j[ok]] + 1e-9))
        out.append((float(d.sum()), float((d * d).sum())))
    return out


def test_tile_constant_and_counts(world):
    w = world
    assert w["sd"].tile >= 4 and w["sd"].tile % 4 == 0
    for b, (c, want) in enumerate(zip(w["cases"], w["want"])):
        got = (int(w["counts"][0, b]), int(w["counts"][1, b]))
        print(f"{c[0]}: {c[5].shape[0]} steps, counted / skipped {got}")
        assert got == (want["steps"], want["skipped"]) == (c[6], c[7]), c[0]


def test_energy_sums_against_fp64(world):
    w = world
    for b, (c, want) in enumerate(zip(w["cases"], w["want"])):
        got = w["sums"][:, b].reshape(3, 5)
        for r, width in enumerate(R.WINDOWS):
            for q in range(3):
                g, t = float(got[r, q]), float(want["sums"][r, q])
                if t == 0.0:
                    assert g == 0.0, (c[0], width, R.SUMS[q])
                    continue
                print(f"{c[0]}, window {width}, sum {R.SUMS[q]}: relative error {abs(g - t) / abs(t):.2e}")
                assert abs(g - t) <= 1e-5 * abs(t), (c[0], width, R.SUMS[q])


def test_log_sums_against_fp32_torch(world):
    """Measured on an MI355X over the 42 sums (7 pairs x 3 windows x {sum d, sum d^2}): the kernel, which transforms in fp64, is
    0 .. 1.2e-13 relative from the oracle; fp32 torch is 7e-9 .. 6e-5 from it; every ratio prints as 0.00 (allowed: 4)."""
    w = world
    over = []
    for b, (c, want) in enumerate(zip(w["cases"], w["want"])):
        got = w["sums"][:, b].reshape(3, 5)
        t32 = _torch32_sums(c[1], c[3], c[5], c[2], c[4])
        for r, width in enumerate(R.WINDOWS):
            for q, name in ((3, "d"), (4, "dd")):
                t = float(want["sums"][r, q])
                err, allowed = abs(float(got[r, q]) - t), abs(t32[r][q - 3] - t)
                print(f"{c[0]}, window {width}, sum {name} = {t:.6e}: error {err:.2e} ({err / abs(t):.1e} relative), fp32 torch {allowed:.2e}, "
                      f"ratio {err / allowed if allowed else float('nan'):.2f}")
                if not err <= 4.0 * allowed:
                    over.append((c[0], width, name, err, allowed))
    assert not over, over


def test_measure_reports_the_oracles_fields(world):
    w = world
    c = w["cases"]
    recs = w["sd"].measure([x[1] for x in c], [x[3] for x in c], [x[5] for x in c], [x[2] for x in c], [x[4] for x in c])
    for b, (rec, x) in enumerate(zip(recs, c)):
        assert rec == R.spectral_metrics(w["sums"][:, b], int(w["counts"][0, b]), int(w["counts"][1, b])), "measure() is run_packed's sums"
        want = R.measure(x[1], x[3], x[5], x[2], x[4])
        print(x[0], {k: (rec[k], want[k]) for k in ("mr_sc_dtw", "mr_lsd_dtw", "level_db_1024")})
        for k in R.FIELDS:
            if want[k] is None:
                assert rec[k] is None, (x[0], k)
            else:
                assert abs(rec[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (x[0], k)
    assert recs[5]["sc_dtw_256"] is None and recs[5]["mr_sc_dtw"] is None and recs[5]["mr_lsd_dtw"] > 0.0
    with pytest.raises(ValueError, match="1023 samples"):
        w["sd"].measure([c[0][1][:1023]], [c[0][3]], [c[0][5]], [5], [7])


def test_a_pair_does_not_depend_on_the_batch(world):
    w = world
    pick = [w["cases"][k] for k in (0, 4, 6)]
    alone = [_run(w["sd"], [c]) for c in pick]
    for order in ((0, 1, 2), (2, 0, 1)):
        sums, counts = _run(w["sd"], [pick[k] for k in order])
        for col, k in enumerate(order):
            assert torch.equal(sums[:, col], alone[k][0][:, 0]) and torch.equal(counts[:, col], alone[k][1][:, 0]), (order, k)
    for n, k in enumerate((0, 4, 6)):
        assert torch.equal(w["sums"][:, k], alone[n][0][:, 0]) and torch.equal(w["counts"][:, k], alone[n][1][:, 0])


# ---- through evaluate() ---------------------------------------------------------------------------------------------------------

VA = "duration_adaptor.variance_adaptor"
STOP_AT_MIN = dict(max_len=160, stop_threshold=0.0)


def _gl():
    return dict(n_iter=2, generator=torch.Generator().manual_seed(5))


@pytest.fixture(scope="module")
def toy():
    """The tiny 80-mel engine of test_evaluate_audio_gpu.py, its mels, and recordings a fifth longer than them."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import kokoro_oracle as O
    from kokoro_ruslan_amd.dtw import MelAligner
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.features import FeatureExtractor
    from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    fx = np.load(os.path.join(GOLDEN, "inference_tiny.npz"))
    dims = [int(x) for x in fx["dims"]]
    dims[1] = 80
    d = O.ModelDims(*dims)
    P = O.init_params(d, int(fx["seed"]))
    g = torch.Generator().manual_seed(int(fx["seed"]) + 1)
    for n, p in P.items():
        if p.dim() == 1:
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    P[f"{VA}.duration_predictor.linear.bias"].fill_(1.5)
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g).cuda() for n in (2, 9, 5)]
    st = [torch.randint(0, 3, (n,), generator=g).cuda() for n in (2, 9, 5)]
    mels, _ = e.generate_stream(ids, st, slots=2, want_info=True, **STOP_AT_MIN)
    refs, ref_pitch, ref_energy, ref_waves = [], [], [], []
    for k, m in enumerate(mels):
        idx = torch.linspace(0, m.shape[0] - 1, int(1.2 * m.shape[0]) + 1).round().long()
        refs.append(m.cpu()[idx] + 0.05 * torch.randn(idx.numel(), m.shape[1], generator=g))
        ref_pitch.append(torch.rand(idx.numel(), generator=g))
        ref_energy.append(torch.rand(idx.numel(), generator=g))
        ref_waves.append(_sig(max(HOP * (idx.numel() - 1), N_FFT), 10 + k))          # frames 0 .. Tb - 1 all lie within the recording
    return dict(e=e, ids=ids, st=st, mels=mels, refs=refs, ref_pitch=ref_pitch, ref_energy=ref_energy, ref_waves=ref_waves,
                voc=GriffinLimVocoder(), ex=FeatureExtractor(), al=MelAligner())


def test_evaluate_reports_the_spectral_fields(toy, world):
    from kokoro.inference.evaluate import SPECTRAL_COUNTS, SPECTRAL_METRICS, evaluate
    t = toy
    kw = dict(slots=2, vocoder=t["voc"], extractor=t["ex"], ref_pitch=t["ref_pitch"], ref_energy=t["ref_energy"], **STOP_AT_MIN)
    recs, summ, audio = evaluate(t["e"], t["ids"], t["st"], t["refs"], vocoder_kwargs=_gl(), ref_waves=t["ref_waves"], want_audio=True, **kw)
    paths = [al["path"] for al in t["al"].align(t["mels"], t["refs"], want_path=True)]
    want = world["sd"].measure(audio, t["ref_waves"], paths, [int(m.shape[0]) for m in t["mels"]], [int(r.shape[0]) for r in t["refs"]])
    for r, x, p, m in zip(recs, want, paths, t["mels"]):
        print({k: r[k] for k in ("frames", "ref_frames", "mr_sc_dtw", "mr_lsd_dtw", "spec_steps", "spec_skipped")})
        assert {k: r[k] for k in SPECTRAL_METRICS + SPECTRAL_COUNTS} == {k: x[k] for k in SPECTRAL_METRICS + SPECTRAL_COUNTS}
        assert r["spec_steps"] == p.shape[0] and r["spec_skipped"] == 0 and r["frames"] == m.shape[0]
        assert all(np.isfinite(r[k]) for k in SPECTRAL_METRICS)
    assert set(SPECTRAL_METRICS) <= set(summ) and not set(SPECTRAL_COUNTS) & set(summ)
    plain, psumm = evaluate(t["e"], t["ids"], t["st"], t["refs"], vocoder_kwargs=_gl(), **kw)
    for r, q in zip(recs, plain):
        assert set(q) == set(r) - set(SPECTRAL_METRICS + SPECTRAL_COUNTS) and {k: r[k] for k in q} == q
    assert set(psumm) == set(summ) - set(SPECTRAL_METRICS)


def test_evaluate_vocoder_on_two_mels(toy):
    from kokoro.inference.evaluate import SPECTRAL_METRICS, evaluate_vocoder
    t = toy
    mels = [m.cpu() for m in t["mels"][1:]]
    waves = [_sig(HOP * m.shape[0], 20 + k) for k, m in enumerate(mels)]
    recs, summ = evaluate_vocoder(t["voc"], mels, waves, vocoder_kwargs=_gl(), aligner=t["al"], names=["a", "b"])
    for r, m in zip(recs, mels):
        print(r)
        assert r["spec_skipped"] == 0 and r["spec_steps"] == r["frames"] == m.shape[0], "the path is the diagonal"
        assert all(np.isfinite(r[k]) and r[k] is not None for k in SPECTRAL_METRICS)
    assert summ["utterances"] == 2 and set(SPECTRAL_METRICS) <= set(summ) and "hit_bound_share" not in summ
