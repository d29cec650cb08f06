"""HifiganVocoder end to end: the whole generator against the torch restatement (kokoro_ruslan_amd.vocoder_torch) for V1 and a
V2-like config in both math modes, bit-exact batch invariance, output lengths, and kokoro-synth --vocoder.

Bounds (relative L2 of the waveform): f32 mode <= 1e-4 against fp64 (measured ~1e-6).  bf16 mode <= 3e-2 against fp64 on
bf16-rounded operands and <= 6e-2 against unrounded fp64 (measured 4e-3 .. 1e-2 for both): ~80 layers of bf16 operands compound, and a
rounding that flips in one layer moves every later one, so rounding the restatement's operands does not bring it much closer."""
import json
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import vocoder_torch as VT
from kokoro_ruslan_amd.vocoder import DEFAULT_CONFIG, HifiganVocoder

pytestmark = pytest.mark.gpu
V2 = {"upsample_rates": [8, 8, 4, 2], "upsample_kernel_sizes": [16, 16, 8, 4], "upsample_initial_channel": 128,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _mels(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(f, 80, generator=g) * 2.0 - 5.0 for f in frames]


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("cfg_name", ["v1", "v2"])
def test_generator_matches_torch_restatement(cfg_name):
    _need_gpu()
    cfg = dict(DEFAULT_CONFIG) if cfg_name == "v1" else V2
    sd = VT.random_state_dict(cfg, seed=7)
    mels = _mels([1, 3, 20], seed=1)
    for mode, tol_r, tol_u in (("f32", 1e-4, 1e-4), ("bf16", 3e-2, 6e-2)):
        voc = HifiganVocoder(cfg, math_mode=mode)
        voc.load_state_dict(sd)
        outs = voc.vocode([m.cuda() for m in mels])
        W = {n: w.double() for n, w in voc.weights.items()}
        for m, o in zip(mels, outs):
            ref = VT.forward(W, voc.biases, cfg, m.double())
            assert o.dtype == torch.float32 and o.shape == (m.shape[0] * voc.hop,) and float(ref.std()) > 0.05
            assert _rel(o.cpu(), ref) <= tol_u, (cfg_name, mode, "unrounded", _rel(o.cpu(), ref))
            if mode == "bf16":
                rr = VT.forward(W, voc.biases, cfg, m.double(), round_bf16=True)
                assert _rel(o.cpu(), rr) <= tol_r, (cfg_name, mode, "rounded", _rel(o.cpu(), rr))


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_batch_invariance_bit_for_bit(mode):
    _need_gpu()
    voc = HifiganVocoder(math_mode=mode)
    voc.load_state_dict(VT.random_state_dict(None, seed=3))
    frames = [1, 2, 3, 17, 40, 9]
    mels = [m.cuda() for m in _mels(frames, seed=2)]
    together = voc.vocode(mels)
    assert [o.shape[0] for o in together] == [256 * f for f in frames]
    perm = [4, 0, 5, 2, 1, 3]
    reordered = voc.vocode([mels[i] for i in perm])
    grouped = voc.vocode(mels, max_samples=256 * 20)          # several groups, one mel (40 frames) above the cap on its own
    for b, m in enumerate(mels):
        alone = voc.vocode([m])[0]
        assert float(alone.std()) > 0.05
        assert torch.equal(together[b], alone), (mode, b)
        assert torch.equal(reordered[perm.index(b)], alone), (mode, b)
        assert torch.equal(grouped[b], alone), (mode, b)


def test_vocode_rejects_bad_mels():
    _need_gpu()
    voc = HifiganVocoder(V2)
    with pytest.raises(RuntimeError, match="no weights"):
        voc.vocode([torch.zeros(3, 80, device="cuda")])
    voc.load_state_dict(VT.random_state_dict(V2, seed=0))
    with pytest.raises(ValueError, match="frames"):
        voc.vocode([torch.zeros(3, 20, device="cuda")])
    with pytest.raises(ValueError, match="frames"):
        voc.vocode([torch.zeros(0, 80, device="cuda")])


def test_kokoro_synth_with_vocoder(tmp_path):
    """kokoro-synth --vocoder DIR (a V1 generator saved as weight_g / weight_v, no config.json: the defaults) writes one 22050 Hz int16
    .wav of 256 * frames samples per utterance, next to .npy mels equal to a run without --vocoder."""
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
    vdir = tmp_path / "hifigan"
    vdir.mkdir()
    sd = VT.random_state_dict(None, seed=11, form="weight_norm")
    torch.save({"generator": sd}, vdir / "generator.pth")
    g = torch.Generator().manual_seed(2)
    utts = {"u0": torch.randint(1, 59, (5,), generator=g), "u1": torch.randint(1, 59, (17,), generator=g),
            "u2": torch.randint(1, 59, (9,), generator=g)}
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps({"name": k, "phoneme_indices": v.tolist()}) + "\n" for k, v in utts.items()))
    common = ["--checkpoint", str(ck), "--ids", str(ids_file), "--batch-size", "2", "--math", "f32", "--max-len", "40", "--weights",
              "model"]
    plain, voiced = tmp_path / "plain", tmp_path / "voiced"
    assert cli.main(common + ["--output", str(plain)]) == 0
    assert cli.main(common + ["--output", str(voiced), "--vocoder", str(vdir), "--vocoder-math", "f32"]) == 0
    assert sorted(os.listdir(plain)) == ["u0.npy", "u1.npy", "u2.npy"]
    assert sorted(os.listdir(voiced)) == ["u0.npy", "u0.wav", "u1.npy", "u1.wav", "u2.npy", "u2.wav"]
    voc = HifiganVocoder(math_mode="f32")
    voc.load_state_dict(sd)
    for k in utts:
        mel = np.load(voiced / f"{k}.npy")
        assert np.array_equal(mel, np.load(plain / f"{k}.npy"))
        sr, data = wavfile.read(str(voiced / f"{k}.wav"))
        assert sr == 22050 and data.dtype == np.int16 and data.shape == (256 * mel.shape[1],)
        want = vocode(voc, [torch.from_numpy(mel).t().contiguous().cuda()])[0].cpu()
        want = (want / want.abs().max()).numpy()
        assert np.abs(data.astype(np.float64) / 32767 - want).max() <= 2.0 / 32767
