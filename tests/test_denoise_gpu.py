"""SpectralDenoiser and kokoro-synth --denoise on the device: the bias of a HiFi-GAN generator (seeded random weights, the smallest
config with the hop of 256 that resolve_config accepts) against the fp64 restatement of its own output, denoising against the
restatement within the kernels' bound (tests/test_denoise_kernels_gpu.py), the argument errors, and the command-line run."""
import json
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import denoise_torch as DT
from kokoro_ruslan_amd import griffinlim_torch as GT
from kokoro_ruslan_amd import vocoder_torch as VT
from kokoro_ruslan_amd.denoise import SpectralDenoiser
from kokoro_ruslan_amd.vocoder import HifiganVocoder

pytestmark = pytest.mark.gpu
SMALL = {"upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 64,
         "resblock_kernel_sizes": [3], "resblock_dilation_sizes": [[1]]}
TOL, EDGE = 1e-5, 768
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def _vocoder():
    if "voc" not in _cache:
        voc = HifiganVocoder(SMALL, math_mode="f32")
        voc.load_state_dict(VT.random_state_dict(SMALL, seed=4))
        _cache["voc"] = voc
    return _cache["voc"]


def _denoiser():
    """(denoiser with the vocoder's bias, the vocoded silent mel)"""
    if "den" not in _cache:
        voc = _vocoder()
        den = SpectralDenoiser()
        assert den.bias is None
        b = den.bias_from_vocoder(voc)
        assert b is den.bias
        silent = voc.vocode([torch.full((88, 80), -11.5, device="cuda")])[0]
        _cache["den"] = (den, silent)
    return _cache["den"]


def test_bias_from_vocoder_matches_fp64():
    _need_gpu()
    den, silent = _denoiser()
    assert silent.shape == (88 * 256,) and float(silent.abs().max()) > 0
    want = DT.bias_from_wave(silent)
    assert den.bias.dtype == torch.float32 and den.bias.shape == (513,) and den.bias.is_cuda
    print(f"bias rel L2 {_rel(den.bias, want):.3e}")
    assert _rel(den.bias, want) <= 1e-5, _rel(den.bias, want)


def test_denoise_lowers_the_silent_mel_and_matches_fp64_on_speech():
    _need_gpu()
    den, silent = _denoiser()
    out = den.denoise([silent])[0]
    assert out.shape == silent.shape and out.dtype == torch.float32
    assert float(out.double().norm()) < float(silent.double().norm())
    speech = _vocoder().vocode([GT.harmonic_logmel(12).float().cuda()])[0]
    got = den.denoise([silent, speech])[1]
    want = DT.denoise(speech, den.bias, float(torch.tensor(0.005, dtype=torch.float32)))
    assert got.shape == want.shape == (12 * 256,)
    errs = (_rel(got, want), _rel(got[:EDGE], want[:EDGE]), _rel(got[-EDGE:], want[-EDGE:]))
    print(f"speech rel L2 whole {errs[0]:.3e} first {errs[1]:.3e} last {errs[2]:.3e}")
    assert max(errs) <= TOL, errs
    assert torch.equal(got, den.denoise([speech])[0]), "the same bits alone"


def test_strength_zero_clones_without_a_launch():
    _need_gpu()
    from kokoro_ruslan_amd import lib as kk
    den, silent = _denoiser()
    before = kk.launches
    out = den.denoise([silent, silent[:1024]], strength=0.0)
    assert kk.launches == before
    assert torch.equal(out[0], silent) and out[0].data_ptr() != silent.data_ptr() and out[1].shape == (1024,)


def test_value_errors():
    _need_gpu()
    den, silent = _denoiser()
    fresh = SpectralDenoiser()
    with pytest.raises(ValueError, match="no bias"):
        fresh.denoise([silent])
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            den.denoise([silent], strength=bad)
    with pytest.raises(ValueError, match="waveform 1"):
        den.denoise([silent, silent[:1023]])
    with pytest.raises(ValueError, match="waveform 0"):
        den.denoise([silent.reshape(2, -1)])
    for bad in (torch.zeros(512), torch.full((513,), -1.0), torch.full((513,), float("nan")), torch.zeros(1, 513)):
        with pytest.raises(ValueError, match="bias"):
            fresh.set_bias(bad)
    assert fresh.bias is None
    fresh.set_bias(torch.zeros(513, dtype=torch.float64))
    assert fresh.bias.dtype == torch.float32 and fresh.bias.is_cuda


def test_kokoro_synth_with_denoise(tmp_path, capsys):
    """kokoro-synth --vocoder DIR --denoise 0.01 writes waveforms that differ from a run without the flag; two runs without it write
    the same bytes."""
    _need_gpu()
    from scipy.io import wavfile
    from kokoro.cli import synth as cli
    from kokoro.inference import denoise, vocode
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
    sd = VT.random_state_dict(SMALL, seed=11, form="weight_norm")
    torch.save({"generator": sd}, vdir / "generator.pth")
    (vdir / "config.json").write_text(json.dumps(SMALL))
    g = torch.Generator().manual_seed(2)
    utts = {"u0": torch.randint(1, 59, (5,), generator=g), "u1": torch.randint(1, 59, (17,), generator=g)}
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps({"name": k, "phoneme_indices": v.tolist()}) + "\n" for k, v in utts.items()))
    common = ["--checkpoint", str(ck), "--ids", str(ids_file), "--batch-size", "2", "--math", "f32", "--max-len", "40", "--weights",
              "model", "--vocoder", str(vdir), "--vocoder-math", "f32"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    assert cli.main(common + ["--output", str(a)]) == 0
    plain_line = capsys.readouterr().out.strip().splitlines()[-1].split(" -> ")[0]
    assert cli.main(common + ["--output", str(b)]) == 0
    assert cli.main(common + ["--output", str(c), "--denoise", "0.01"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1].split(" -> ")[0]
    assert "denoised at strength 0.01" in line and "denois" not in plain_line and "(f32 vocoder)" in plain_line
    assert sorted(os.listdir(a)) == sorted(os.listdir(c)) == ["u0.npy", "u0.wav", "u1.npy", "u1.wav"]
    voc = HifiganVocoder(SMALL, math_mode="f32")
    voc.load_state_dict(sd)
    den = SpectralDenoiser()
    den.bias_from_vocoder(voc)
    for k in utts:
        assert (a / f"{k}.wav").read_bytes() == (b / f"{k}.wav").read_bytes()
        assert (a / f"{k}.npy").read_bytes() == (c / f"{k}.npy").read_bytes()
        (sr, plain), (sr2, den_wav) = wavfile.read(str(a / f"{k}.wav")), wavfile.read(str(c / f"{k}.wav"))
        assert sr == sr2 == 22050 and plain.shape == den_wav.shape and den_wav.dtype == np.int16
        assert not np.array_equal(plain, den_wav)
        mel = torch.from_numpy(np.load(c / f"{k}.npy")).t().contiguous().cuda()
        want = denoise(den, vocode(voc, [mel]), 0.01)[0].cpu()
        want = (want / want.abs().max()).numpy()
        assert np.abs(den_wav.astype(np.float64) / 32767 - want).max() <= 2.0 / 32767
