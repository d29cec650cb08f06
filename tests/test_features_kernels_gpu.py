"""The feature kernels (csrc/kk_features.hip) one stage at a time against features_torch in fp64 on the same fp32 input: the
linear mel power (whole utterance and its reflected edge frames), the log-mel, the per-frame energy term, and what the pitch
kernel writes before any decision is taken.  The ragged batch of tests/golden/features.npz plus an all-zero utterance, in one call.

Bounds: linear mel relative L2 <= 1e-5 per utterance (the bound of the other fp32 FFT kernels here; fp32 torch.stft: 0.8e-6 .. 2.0e-6).
Log-mel: the maximum absolute error is dominated by near-silent bins, so the kernels are allowed 4x what fp32 features_torch itself
shows against fp64 on the same utterance.  Autocorrelation maximum and mean square: 1e-5 relative per frame; candidate frequency
within 0.075 Hz (1e-4 of the normalised range) on at least 99 % of the frames.

Measured on an MI355X, per utterance (700 / 3000 / 33000 / 77000 / 143000 samples): linear mel 0.9e-7 .. 1.2e-7 whole and on the edge
frames; log-mel maximum error / fp32 torch's own: 1.33, 0.49, 0.72, 0.85, 0.33 (errors 6.3e-6 .. 6.3e-5).
"""
import numpy as np
import os
import pytest
import torch

from kokoro_ruslan_amd import features_torch as FT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features.npz")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _waves():
    g = np.load(GOLDEN)
    return [torch.from_numpy(g[f"signal_{i}"]).float() / 32768.0 for i in range(len(g["lengths"]))] + [torch.zeros(5000)]


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def _rel_per_frame(got, ref):
    """Largest relative error over the frames; a frame that lies wholly in the zero padding (reference exactly 0) must be exactly 0."""
    got = got.double().cpu()
    zero = ref == 0
    assert bool((got[zero] == 0).all())
    return float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max())


@pytest.fixture(scope="module")
def run():
    _need_gpu()
    from kokoro_ruslan_amd.features import FeatureExtractor
    waves = _waves()
    got = FeatureExtractor().extract([w.cuda() for w in waves], keep_linear=True, intermediates=True)
    want = [FT.extract(w, dtype=torch.float64) for w in waves]
    return waves, got, want


def test_linear_mel_power(run):
    waves, got, want = run
    for b, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert g["mel_linear"].shape == w["mel_linear"].shape and g["mel_linear"].dtype == torch.float32
        whole = _rel(g["mel_linear"], w["mel_linear"])
        edge = [0, 1, -2, -1]
        edges = _rel(g["mel_linear"][:, edge], w["mel_linear"][:, edge])
        print(f"utterance {b}: linear mel relative L2 {whole:.2e}, edge frames {edges:.2e}")
        assert whole <= 1e-5 and edges <= 1e-5, (b, whole, edges)


def test_logmel_against_fp32_torch(run):
    """Measured ratios kernel / fp32 torch on an MI355X: 1.33, 0.49, 0.72, 0.85, 0.33 (allowed: 4)."""
    waves, got, want = run
    for b, (x, g, w) in enumerate(zip(waves[:-1], got[:-1], want[:-1])):
        t32 = FT.extract(x, dtype=torch.float32)["mel_spec"]
        allowed = float((t32.double() - w["mel_spec"]).abs().max())
        err = float((g["mel_spec"].double().cpu() - w["mel_spec"]).abs().max())
        print(f"utterance {b}: log-mel max error {err:.2e}, fp32 torch {allowed:.2e}, ratio {err / allowed:.2f}")
        assert err <= 4.0 * allowed, (b, err, allowed)


def test_energy_term(run):
    waves, got, want = run
    for b, (g, w) in enumerate(zip(got, want)):
        raw = torch.log1p(w["mel_linear"].mean(0))
        e = torch.log1p(g["mel_linear"].double().cpu().mean(0))
        assert float((e - raw).abs().max()) <= 1e-5 * max(1.0, float(raw.max())), b


def test_pitch_intermediates(run):
    waves, got, want = run
    total = bad = 0
    for b, (x, g) in enumerate(zip(waves[:-1], got[:-1])):
        cand, acmax, msq = FT.pitch_candidates(FT.normalise(x, torch.float64))
        assert g["pitch_candidate"].shape == cand.shape == (FT.pitch_frames(x.shape[0]),)
        ra, rm = _rel_per_frame(g["pitch_acmax"], acmax), _rel_per_frame(g["pitch_msq"], msq)
        off = (g["pitch_candidate"].double().cpu() - cand).abs() > 0.075
        print(f"utterance {b}: acmax relative {ra:.2e}, mean square relative {rm:.2e}, candidates out of bound {int(off.sum())} / {off.numel()}")
        assert ra <= 1e-5 and rm <= 1e-5, (b, ra, rm)
        total += off.numel()
        bad += int(off.sum())
    assert bad <= 0.01 * total, (bad, total)


def test_all_zero_intermediates(run):
    waves, got, want = run
    g = got[-1]
    assert float(g["pitch_acmax"].abs().max()) == 0.0 and float(g["pitch_msq"].abs().max()) == 0.0
    assert torch.equal(g["mel_linear"], torch.zeros_like(g["mel_linear"]))
