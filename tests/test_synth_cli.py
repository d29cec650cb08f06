"""kokoro-synth and kokoro.inference.synth: inference-control resolution (inference/inference.py:393-452, 552-562), the --trim rule
(:588-619), argument parsing and the --ids reader on the CPU; one end-to-end run on the GPU."""
import json
import os
import types

import numpy as np
import pytest
import torch

from kokoro.cli import synth as cli
from kokoro.inference.synth import pick_weights, resolve_controls, trim_trailing_silence


def test_controls_default_without_metadata_or_config():
    c = resolve_controls({})
    assert (c.max_len, c.stop_threshold, c.min_len_ratio, c.min_len_floor) == (1200, 0.45, 0.7, 12)
    assert c.post_expected_stop_threshold is None and "post_expected_stop_threshold" not in c.kwargs()


def test_controls_metadata_before_config_before_defaults():
    cfg = types.SimpleNamespace(inference_max_len=900, inference_stop_threshold=0.3, inference_min_len_ratio=None)
    ck = {"config": cfg, "model_metadata": {"inference_controls": {"max_len": 700, "min_len_floor": 20}}}
    c = resolve_controls(ck)
    assert c.max_len == 700              # metadata
    assert c.stop_threshold == 0.3       # config
    assert c.min_len_ratio == 0.7        # config field None -> default
    assert c.min_len_floor == 20         # metadata


def test_controls_clamps():
    ck = {"model_metadata": {"inference_controls": {"max_len": 10, "stop_threshold": 5.0, "min_len_ratio": 0.01, "min_len_floor": -3}}}
    c = resolve_controls(ck)
    assert (c.max_len, c.stop_threshold, c.min_len_ratio, c.min_len_floor) == (64, 0.99, 0.1, 1)
    c = resolve_controls({"model_metadata": {"inference_controls": {"stop_threshold": 0.0, "min_len_ratio": 9, "max_len": "x"}}})
    assert (c.stop_threshold, c.min_len_ratio, c.max_len) == (0.05, 1.5, 1200)


def test_controls_explicit_values_win_and_threshold_sets_post():
    ck = {"model_metadata": {"inference_controls": {"max_len": 700, "stop_threshold": 0.6}}}
    c = resolve_controls(ck, max_len=30, stop_threshold=0.01, min_len_floor=2)
    assert (c.max_len, c.stop_threshold, c.min_len_floor) == (30, 0.01, 2)      # explicit: not clamped
    assert c.post_expected_stop_threshold == 0.01 and c.kwargs()["post_expected_stop_threshold"] == 0.01


def test_pick_weights():
    m, e = {"a": torch.zeros(1)}, {"a": torch.ones(1)}
    assert pick_weights({"model_state_dict": m, "ema_model_state_dict": e})[1] == "ema"
    assert pick_weights({"model_state_dict": m, "ema_model_state_dict": e}, "model")[0] is m
    assert pick_weights({"model_state_dict": m}) == (m, "model")
    with pytest.raises(RuntimeError):
        pick_weights({"model_state_dict": m}, "ema")
    with pytest.raises(ValueError):
        pick_weights({"model_state_dict": m}, "best")


def _mel(means):
    return torch.tensor(means, dtype=torch.float32)[:, None].repeat(1, 80)


def test_trim_cuts_the_trailing_silence_with_a_margin():
    mel = _mel([-5.0] * 100 + [-11.0] * 100)           # q10 = q20 = -5: threshold clamps to -9.2; last voiced frame 99
    out = trim_trailing_silence(mel)
    assert out.shape == (124, 80)                       # 99 + 24 + 1
    assert torch.equal(out, mel[:124])


def test_trim_keeps_at_least_60_frames_and_clamps():
    mel = _mel([3.0] * 10 + [-20.0] * 90)               # clamped to [-11.5, 2]; last voiced 9 -> end 34 -> kept 60
    out = trim_trailing_silence(mel)
    assert out.shape[0] == 60 and float(out.max()) == 2.0 and float(out.min()) == -11.5


def test_trim_adaptive_threshold_and_no_voiced_frame():
    # quiet utterance: q10 / q20 of the frame means around -10.5 -> threshold clamps to -9.8; -9.5 counts as voiced
    mel = _mel([-10.5] * 50 + [-9.5] * 10 + [-10.5] * 140)
    assert trim_trailing_silence(mel).shape[0] == 59 + 24 + 1
    silent = _mel([-11.0] * 80)
    assert trim_trailing_silence(silent).shape[0] == 80, "no voiced frame: no trim"
    assert trim_trailing_silence(torch.zeros(0, 80)).shape == (0, 80)


def test_parser():
    a = cli.build_parser().parse_args(["--checkpoint", "c.pth", "--ids", "x.jsonl", "--output", "o"])
    assert (a.batch_size, a.weights, a.math, a.trim, a.stop_threshold, a.max_len) == (32, "auto", "bf16", False, None, None)
    a = cli.build_parser().parse_args(["--checkpoint", "c", "--features", "cache", "--indices", "3", "5", "--output", "o",
                                       "--batch-size", "8", "--weights", "ema", "--stop-threshold", "0.3", "--max-len", "500",
                                       "--min-len-ratio", "0.5", "--min-len-floor", "4", "--trim", "--math", "f32"])
    assert (a.features, a.indices, a.batch_size, a.weights, a.stop_threshold, a.max_len, a.min_len_ratio, a.min_len_floor, a.trim,
            a.math) == ("cache", [3, 5], 8, "ema", 0.3, 500, 0.5, 4, True, "f32")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--checkpoint", "c", "--ids", "x", "--features", "y", "--output", "o"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--checkpoint", "c", "--output", "o"])


def test_read_ids(tmp_path):
    p = tmp_path / "u.jsonl"
    p.write_text('{"name": "a", "phoneme_indices": [3, 4, 5], "stress_indices": [0, 1, 0]}\n\n'
                 '{"name": "b", "phoneme_indices": [7], "stress_indices": [2]}\n')
    names, ids, st = cli.read_ids(str(p))
    assert names == ["a", "b"] and ids[0].tolist() == [3, 4, 5] and st[1].tolist() == [2] and ids[0].dtype == torch.int64
    p.write_text('{"name": "a", "phoneme_indices": [3]}\n{"name": "b", "phoneme_indices": [4, 5]}\n')
    assert cli.read_ids(str(p))[2] is None
    p.write_text('{"name": "a", "phoneme_indices": [3], "stress_indices": [1]}\n{"name": "b", "phoneme_indices": [4]}\n')
    with pytest.raises(ValueError):
        cli.read_ids(str(p))
    p.write_text('{"name": "a", "phoneme_indices": [3]}\n{"name": "a", "phoneme_indices": [4]}\n')
    with pytest.raises(ValueError):
        cli.read_ids(str(p))


@pytest.mark.gpu
def test_kokoro_synth_end_to_end(tmp_path):
    """A checkpoint written by kokoro.training.checkpoint at tiny dims -> kokoro-synth -> one [n_mels, frames_b] .npy per utterance,
    equal to generate() on that utterance alone."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.training.checkpoint import save_checkpoint
    from kokoro.training.config import TrainingConfig
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d = ModelDims(vocab=59, mel=20, hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32, var_kernel=3,
                  var_bins=16, max_len=300)
    e = KokoroEngine(d, StepHyper(), math_mode="f32", total_steps=100, seed=5)
    cfg = TrainingConfig(n_mels=20, hidden_dim=128, n_encoder_layers=1, n_decoder_layers=1, n_heads=2, encoder_ff_dim=96,
                         decoder_ff_dim=96, max_decoder_seq_len=300, variance_filter_size=32, n_variance_bins=16)
    ck = save_checkpoint(e, cfg, 0, 1.0, str(tmp_path / "ck"))
    g = torch.Generator().manual_seed(2)
    utts = {"u0": torch.randint(1, 59, (5,), generator=g), "u1": torch.randint(1, 59, (17,), generator=g),
            "u2": torch.randint(1, 59, (9,), generator=g)}
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps({"name": k, "phoneme_indices": v.tolist()}) + "\n" for k, v in utts.items()))
    out = tmp_path / "mels"
    assert cli.main(["--checkpoint", ck, "--ids", str(ids_file), "--output", str(out), "--batch-size", "2", "--math", "f32",
                     "--max-len", "40", "--weights", "model"]) == 0
    kw = dict(max_len=40, stop_threshold=0.45, min_len_ratio=0.7, min_len_floor=12)
    for k, v in utts.items():
        a = np.load(out / f"{k}.npy")
        ref = e.generate(v[None].cuda(), **kw)[0].cpu()
        assert a.dtype == np.float32 and a.shape == (20, ref.shape[0])
        np.testing.assert_allclose(a, ref.t().numpy(), atol=1e-4, rtol=0)
    assert sorted(os.listdir(out)) == ["u0.npy", "u1.npy", "u2.npy"]
