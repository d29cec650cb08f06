"""GriffinLimVocoder end to end: the whole algorithm against the fp64 torch restatement (kokoro_ruslan_amd.griffinlim_torch) with the
same initial phases, momentum 0, phase-0 init, bit-exact batch invariance, output lengths, the reference's seeded random phases, and
kokoro-synth --griffin-lim.

Bounds (relative L2 of the waveform against fp64): <= 1e-4 up to 16 iterations over the batch (and per utterance up to 4; 1e-3 per
utterance at 16, where the 4-frame one measured 3.8e-4); <= 3e-2 at 60, where fp32 on the CPU drifts to ~1e-3
(Griffin-Lim amplifies rounding: the phase retrieval has many near-equivalent fixed points), with the spectral convergence within 1e-3
of fp64's."""
import json
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import griffinlim_torch as GT
from kokoro_ruslan_amd.griffinlim import N_BINS, GriffinLimVocoder, random_angles

pytestmark = pytest.mark.gpu
FRAMES = [300, 4, 7, 64, 1001]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def _mels(frames=FRAMES, seed=0):
    return [GT.harmonic_logmel(f, seed=seed + i, f0=100.0 + 15 * i).float() for i, f in enumerate(frames)]


def _angles(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((N_BINS, f), dtype=torch.complex64, generator=g) for f in frames]


@pytest.mark.parametrize("n_iter", [0, 1, 4, 16])
def test_matches_fp64_restatement(n_iter):
    _need_gpu()
    voc = GriffinLimVocoder()
    mels, ang = _mels(), _angles(FRAMES, 1)
    outs = voc.vocode([m.cuda() for m in mels], n_iter=n_iter, angles=ang)
    got, refs = [], []
    for m, a, o in zip(mels, ang, outs):
        ref = GT.vocode(m.double(), a, n_iter=n_iter)
        assert o.dtype == torch.float32 and o.shape == ref.shape == (256 * (m.shape[0] - 1),)
        got.append(o.cpu())
        refs.append(ref)
    per = [_rel(o, r) for o, r in zip(got, refs)]
    print(f"n_iter {n_iter}: relative L2 per utterance {['%.1e' % e for e in per]}")
    assert _rel(torch.cat(got), torch.cat(refs)) <= 1e-4, per
    # a 4-frame utterance is all edge and Griffin-Lim amplifies rounding; fp32 torch drifts 4.6e-5 from fp64 on it at 16 iterations
    assert max(per) <= (1e-4 if n_iter <= 4 else 1e-3), per


def test_sixty_iterations_converge_like_fp64():
    _need_gpu()
    voc = GriffinLimVocoder()
    frames = [300, 64]
    mels, ang = _mels(frames, seed=4), _angles(frames, 2)
    outs = voc.vocode([m.cuda() for m in mels], angles=ang)
    for m, a, o in zip(mels, ang, outs):
        S = GT.magnitude(m.double())
        ref = GT.griffinlim(S, a, 60)
        assert _rel(o.cpu(), ref) <= 3e-2, (m.shape[0], _rel(o.cpu(), ref))
        sc, sc_ref = GT.spectral_convergence(o.cpu(), S), GT.spectral_convergence(ref, S)
        assert abs(sc - sc_ref) <= 1e-3 and sc < 0.5, (sc, sc_ref)


def test_momentum_zero():
    _need_gpu()
    voc = GriffinLimVocoder()
    mels, ang = _mels([40, 9], seed=7), _angles([40, 9], 3)
    outs = voc.vocode([m.cuda() for m in mels], angles=ang, momentum=0.0, n_iter=8)
    for i, (m, o) in enumerate(zip(mels, outs)):
        ref = GT.vocode(m.double(), ang[i], n_iter=8, momentum=0.0)
        assert _rel(o.cpu(), ref) <= 1e-4, (i, _rel(o.cpu(), ref))


def test_init_ones():
    """Phase 0 everywhere (rand_init=False).  The start is ill-conditioned: the zero-phase frames give rebuilt spectra whose tiny
    imaginary parts are rounding, so after one iteration fp32 torch is already 1e-2 .. 4e-2 from fp64 (0.19 after eight).  So the
    waveform is checked at n_iter = 0, and after iterations the spectral convergence, the quantity Griffin-Lim minimises."""
    _need_gpu()
    voc = GriffinLimVocoder()
    mels = _mels([40, 9], seed=7)
    for n_iter in (0, 8):
        outs = voc.vocode([m.cuda() for m in mels], init="ones", momentum=0.0, n_iter=n_iter)
        for i, (m, o) in enumerate(zip(mels, outs)):
            ref = GT.vocode(m.double(), None, n_iter=n_iter, momentum=0.0)
            if n_iter == 0:
                assert _rel(o.cpu(), ref) <= 1e-5, (i, _rel(o.cpu(), ref))
            else:
                S = GT.magnitude(m.double())
                sc, sc_ref = GT.spectral_convergence(o.cpu(), S), GT.spectral_convergence(ref, S)
                assert abs(sc - sc_ref) <= 1e-2, (i, sc, sc_ref)


def test_batch_invariance_bit_for_bit():
    _need_gpu()
    voc = GriffinLimVocoder()
    frames = [4, 300, 5, 17, 64, 9, 7]
    mels = [m.cuda() for m in _mels(frames, seed=11)]
    ang = _angles(frames, 5)
    together = voc.vocode(mels, n_iter=6, angles=ang)
    assert [o.shape[0] for o in together] == [256 * (f - 1) for f in frames]
    perm = [3, 6, 0, 5, 1, 4, 2]
    reordered = voc.vocode([mels[i] for i in perm], n_iter=6, angles=[ang[i] for i in perm])
    grouped = voc.vocode(mels, n_iter=6, angles=ang, max_frames=40)      # several groups; the 300- and 64-frame mels each alone
    for b, m in enumerate(mels):
        alone = voc.vocode([m], n_iter=6, angles=[ang[b]])[0]
        assert float(alone.std()) > 1e-3
        assert torch.equal(together[b], alone), b
        assert torch.equal(reordered[perm.index(b)], alone), b
        assert torch.equal(grouped[b], alone), b


def test_random_init_is_the_reference_draw():
    """init="random" under a seeded generator draws torch.rand((1, 513, T_b), complex64) per utterance in input order, as the reference
    does when it vocodes the utterances one by one after the same seed."""
    _need_gpu()
    voc = GriffinLimVocoder()
    frames = [12, 5, 30]
    mels = _mels(frames, seed=2)
    outs = voc.vocode([m.cuda() for m in mels], n_iter=3, generator=torch.Generator().manual_seed(1234))
    g = torch.Generator().manual_seed(1234)
    draws = [torch.rand((1, N_BINS, f), dtype=torch.complex64, generator=g)[0] for f in frames]
    same = voc.vocode([m.cuda() for m in mels], n_iter=3, angles=draws)
    for b, (m, o) in enumerate(zip(mels, outs)):
        assert torch.equal(o, same[b]), b
        assert _rel(o.cpu(), GT.vocode(m.double(), draws[b], n_iter=3)) <= 1e-4, b
    torch.manual_seed(99)
    glob = voc.vocode([m.cuda() for m in mels], n_iter=3)
    torch.manual_seed(99)
    assert all(torch.equal(o, s) for o, s in zip(glob, voc.vocode([m.cuda() for m in mels], n_iter=3, angles=random_angles(frames))))


def test_kokoro_synth_with_griffin_lim(tmp_path):
    """kokoro-synth --griffin-lim writes one 22050 Hz int16 .wav of 256 (frames - 1) samples per utterance, next to .npy mels equal to
    a run without the flag; the waveform is GriffinLimVocoder's on the saved mel with the seeded phases."""
    _need_gpu()
    from scipy.io import wavfile
    from kokoro.cli import synth as cli
    from kokoro.inference import vocode
    from kokoro.training.checkpoint import save_checkpoint
    from kokoro.training.config import TrainingConfig
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d = ModelDims(vocab=59, mel=80, hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32, var_kernel=3,
                  var_bins=16, max_len=300)
    e = KokoroEngine(d, StepHyper(), math_mode="f32", total_steps=100, seed=5)
    cfg = TrainingConfig(n_mels=80, hidden_dim=128, n_encoder_layers=1, n_decoder_layers=1, n_heads=2, encoder_ff_dim=96,
                         decoder_ff_dim=96, max_decoder_seq_len=300, variance_filter_size=32, n_variance_bins=16)
    ck = save_checkpoint(e, cfg, 0, 1.0, str(tmp_path / "ck"))
    g = torch.Generator().manual_seed(2)
    utts = {"u0": torch.randint(1, 59, (5,), generator=g), "u1": torch.randint(1, 59, (17,), generator=g),
            "u2": torch.randint(1, 59, (9,), generator=g)}
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps({"name": k, "phoneme_indices": v.tolist()}) + "\n" for k, v in utts.items()))
    common = ["--checkpoint", str(ck), "--ids", str(ids_file), "--batch-size", "2", "--math", "f32", "--max-len", "40", "--min-len-floor",
              "8", "--weights", "model"]
    plain, voiced = tmp_path / "plain", tmp_path / "voiced"
    assert cli.main(common + ["--output", str(plain)]) == 0
    assert cli.main(common + ["--output", str(voiced), "--griffin-lim", "--griffin-lim-iters", "5", "--griffin-lim-seed", "7"]) == 0
    assert sorted(os.listdir(plain)) == ["u0.npy", "u1.npy", "u2.npy"]
    assert sorted(os.listdir(voiced)) == ["u0.npy", "u0.wav", "u1.npy", "u1.wav", "u2.npy", "u2.wav"]
    mels = [torch.from_numpy(np.load(voiced / f"{k}.npy")).t().contiguous() for k in utts]
    for k, mel in zip(utts, mels):
        assert np.array_equal(mel.t().numpy(), np.load(plain / f"{k}.npy"))
    want = vocode(GriffinLimVocoder(), [m.cuda() for m in mels], n_iter=5, generator=torch.Generator().manual_seed(7))
    for k, mel, w in zip(utts, mels, want):
        sr, data = wavfile.read(str(voiced / f"{k}.wav"))
        assert sr == 22050 and data.dtype == np.int16 and data.shape == (256 * (mel.shape[0] - 1),)
        w = w.cpu()
        w = (w / w.abs().max()).numpy()
        assert np.abs(data.astype(np.float64) / 32767 - w).max() <= 2.0 / 32767
