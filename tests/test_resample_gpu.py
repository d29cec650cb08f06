"""The resampling kernel (csrc/kk_resample.hip) through Resampler against resample_torch in fp64 on the same fp32 input, and the
speed-perturbation path through FeatureExtractor.extract_perturbed.

Inputs: the first four signals of tests/golden/features.npz (700, 3000, 33000 and 77000 samples), a one-sample utterance and an
all-zero one, all rows in ONE call; the short ones under every rate pair below, the two long ones under a coprime pair and a
large-ratio pair each: 22050 -> 19845 (10:9), -> 24255 (10:11), -> 20947 and -> 22793
(coprime), 44100 -> 22050 (2:1, width 13), 48000 -> 22050 (320:147, width 14), 16000 -> 22050 (320:441).

Bound: relative L2 per utterance <= 1e-5 against the fp64 definition, the bound every fp32 signal kernel here carries, on the whole
signal and separately on the first and the last 32 outputs, where the zero edges matter.  The test prints that distance and, beside
it, the distance of torchaudio's own fp32 operation order (resample_torch order="torchaudio") from the same fp64 result: the size of
the deliberate divergence from the reference's arithmetic, recorded and not asserted.  On the CPU's fp32 restatement that second
distance is 1.8e-7 for 10:9 and 10:11, 3.6e-4 for 22050 -> 20947, 3.8e-4 for 22050 -> 22793 and 1.9e-4 for 22050 -> 22047; the
integer-phase order sits at 1.1e-7 (DESIGN §5 "Resampling").
"""
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import resample_torch as RT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "features.npz")
PAIRS = [(22050, 19845), (22050, 24255), (22050, 20947), (22050, 22793), (44100, 22050), (48000, 22050), (16000, 22050)]
LONG = {2: [PAIRS[2], PAIRS[5]], 3: [PAIRS[3], PAIRS[6]]}       # the two long signals (33 and 76+ tiles) take two pairs each: the fp64 reference of a
BOUND = 1e-5                                                   # long row costs a second on the host, and tiling does not depend on the pair


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _signals():
    g = np.load(GOLDEN)
    sig = [torch.from_numpy(g[f"signal_{i}"]).float() / 32768.0 for i in range(4)]
    assert [s.shape[0] for s in sig] == [700, 3000, 33000, 77000]
    return sig + [torch.tensor([0.37]), torch.zeros(5000)]


@pytest.fixture(scope="module")
def case():
    """(waves, orig rates, new rates, the fp64 reference per row): every signal under every rate pair, computed once."""
    _need_gpu()
    waves, of, nf = [], [], []
    for i, s in enumerate(_signals()):
        for o, n in (PAIRS if i not in LONG else LONG[i]):
            waves.append(s)
            of.append(o)
            nf.append(n)
    want = [RT.resample(w, o, n, dtype=torch.float64) for w, o, n in zip(waves, of, nf)]
    return waves, of, nf, want


@pytest.fixture(scope="module")
def got(case):
    _need_gpu()
    from kokoro_ruslan_amd.resample import Resampler
    waves, of, nf, _ = case
    return [y.cpu() for y in Resampler().resample([w.cuda() for w in waves], of, nf)]


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def test_lengths_and_accuracy_against_fp64(case, got):
    _need_gpu()
    waves, of, nf, want = case
    worst = 0.0
    for b, (w, o, n, y, ref) in enumerate(zip(waves, of, nf, got, want)):
        L = w.shape[0]
        assert y.dtype == torch.float32 and y.shape == ((n * L + o - 1) // o,) == ref.shape, (b, y.shape, ref.shape)
        if not bool(w.any()):
            assert torch.equal(y, torch.zeros_like(y)), b              # zeros in, exact zeros out
            continue
        ta = _rel(RT.resample(w, o, n, dtype=torch.float32, order="torchaudio"), ref)
        whole, head, tail = _rel(y, ref), _rel(y[:32], ref[:32]), _rel(y[-32:], ref[-32:])
        print(f"row {b}: {L} samples {o} -> {n}: kernel {whole:.2e} (first 32 {head:.2e}, last 32 {tail:.2e}); "
              f"torchaudio's fp32 order {ta:.2e}")
        worst = max(worst, whole, head, tail)
        assert whole <= BOUND and head <= BOUND and tail <= BOUND, (b, o, n, whole, head, tail)
    print(f"worst relative L2: {worst:.2e}")


def test_batch_invariance_bit_for_bit(case, got):
    _need_gpu()
    from kokoro_ruslan_amd.resample import Resampler
    rs = Resampler()
    waves, of, nf, _ = case
    dev = [w.cuda() for w in waves]
    rev = rs.resample(dev[::-1], of[::-1], nf[::-1])[::-1]
    grouped = rs.resample(dev, of, nf, max_samples=40000)
    for b in range(len(dev)):
        alone = rs.resample([dev[b]], of[b], nf[b])[0].cpu()
        assert torch.equal(got[b], alone), b
        assert torch.equal(rev[b].cpu(), alone), b
        assert torch.equal(grouped[b].cpu(), alone), b


def test_equal_rates_and_argument_checks():
    _need_gpu()
    from kokoro_ruslan_amd.resample import Resampler
    rs = Resampler()
    x = _signals()[1].cuda()
    same, moved = rs.resample([x, x], [22050, 22050], [22050, 19845])
    assert same is x and moved.shape == (2700,)
    both = rs.resample([x, x], 22050, [22050, 19845], normalise=True)
    assert torch.equal(both[0], (x / (x.abs().max() + 1e-9)) / ((x / (x.abs().max() + 1e-9)).abs().max() + 1e-9))
    with pytest.raises(ValueError, match="waveform 1"):
        rs.resample([x, torch.zeros(2, 30)], 22050, 19845)
    with pytest.raises(ValueError, match="waveform 0"):
        rs.resample([torch.zeros(0)], 22050, 19845)
    with pytest.raises(ValueError, match="new_freq"):
        rs.resample([x], 22050, [19845, 19845])
    with pytest.raises(ValueError, match="sample rate"):
        rs.resample([x], 22050, 0)
    with pytest.raises(ValueError, match="outside the kernel's range"):
        rs.resample([x], 22050 * 40, 22050)


FACTORS = [0.9, 1.1, 0.95, 1.0337, 1.0999, 1.0]


def test_speed_perturb_is_peak_resample_peak():
    _need_gpu()
    from kokoro_ruslan_amd.resample import Resampler
    rs = Resampler()
    dev = [w.cuda() for w in _signals()]
    got = rs.speed_perturb(dev, FACTORS)
    for b, (x, f) in enumerate(zip(dev, FACTORS)):
        a = x / (x.abs().max() + 1e-9)
        r = rs.resample([a], 22050, int(22050 * f))[0]
        want = r / (r.abs().max() + 1e-9)
        assert got[b].shape == want.shape == (RT.resampled_length(x.shape[0], 22050, int(22050 * f)),)
        assert torch.equal(got[b], want), (b, f)
        if bool(x.any()):
            assert abs(float(got[b].abs().max()) - 1.0) < 1e-6
            ref = RT.speed_perturb(x.cpu(), f)
            assert _rel(got[b].cpu(), ref) <= BOUND, (b, f)


def test_extract_perturbed_is_extract_of_speed_perturb():
    _need_gpu()
    from kokoro_ruslan_amd.features import FeatureExtractor
    from kokoro_ruslan_amd.resample import Resampler
    ext = FeatureExtractor()
    dev = [w.cuda() for w in _signals()]
    got = ext.extract_perturbed(dev, FACTORS)
    want = ext.extract(Resampler().speed_perturb(dev, FACTORS))
    grouped = ext.extract_perturbed(dev, FACTORS, max_samples=40000)
    short = ext.extract_perturbed(dev, FACTORS, max_seq_length=64)
    for b, (g, w) in enumerate(zip(got, want)):
        n = RT.resampled_length(dev[b].shape[0], 22050, int(22050 * FACTORS[b]))
        assert g["mel_length"] == w["mel_length"] == min(1 + max(n, 1024) // 256, 1800), b
        assert short[b]["mel_length"] == min(g["mel_length"], 64)
        for k in ("mel_spec", "pitch", "energy"):
            assert torch.equal(g[k], w[k]), (b, k)
            assert torch.equal(grouped[b][k], w[k]), (b, k)
    assert float(got[3]["pitch"].max()) > 0.0 and float(got[3]["energy"].std()) > 1e-3
    with pytest.raises(ValueError, match="factors"):
        ext.extract_perturbed(dev, FACTORS[:2])
