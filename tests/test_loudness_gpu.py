"""LoudnessNormaliser end to end on the device: a ragged batch against the fp64 oracle, kokoro.inference.normalise_loudness, the
argument errors, `kokoro-synth --griffin-lim --loudness` and `kokoro-precompute --trim-silence --loudness --conditioned-wavs`."""
import json
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import loudness_torch as LT

pytestmark = pytest.mark.gpu
FS = 22050
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _norm():
    from kokoro_ruslan_amd.loudness import LoudnessNormaliser
    if "n" not in _cache:
        _cache["n"] = LoudnessNormaliser()
    return _cache["n"]


def _speechlike(n: int, seed: int, level: float, lead: int, tail: int) -> torch.Tensor:
    """lead samples of faint noise | a swelling two-tone with noise at `level` | tail samples of faint noise"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / FS
    x = level * (torch.sin(2 * math.pi * (200 + 30 * seed) * t) + 0.3 * torch.sin(2 * math.pi * 1700 * t)
                 + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)) * (0.5 + 0.5 * torch.sin(2 * math.pi * 2.0 * t) ** 2)
    faint = 3e-5 * torch.randn(n, generator=g, dtype=torch.float64)
    x[:lead] = faint[:lead]
    x[n - tail:] = faint[n - tail:]
    return x.to(torch.float32)


def _batch():
    if "b" not in _cache:
        _cache["b"] = [_speechlike(30011, 1, 0.2, 6000, 4000), _speechlike(4000, 2, 0.1, 500, 500), _speechlike(52345, 3, 0.02, 9000, 12000),
                       _speechlike(16000, 4, 0.5, 0, 3000)]
        _cache["b"][2][20000] = 0.9                               # a click: the gain to the target would take it over full scale
    return _cache["b"]


def test_normalise_ragged_batch_end_to_end():
    _need_gpu()
    waves = _batch()
    out, info = _norm().normalise([w.cuda() for w in waves], target_lufs=-20.0, peak_db=-1.0, trim_db=40.0)
    assert len(out) == len(info) == 4
    again = _norm().measure(out)
    for w, y, i, L2 in zip(waves, out, info, again):
        _, want = LT.normalise(w, -20.0, -1.0, trim=40.0)
        assert want["trim_margin"] >= 0.01 and want["gate_margin"] >= 0.01
        assert (i["start"], i["end"]) == (want["start"], want["end"]) and y.shape == (i["end"] - i["start"],) and y.is_cuda
        assert i["limited"] == want["limited"]
        if want["measured"] is None:
            assert i["measured"] is None and i["gain"] == 1.0 and L2 is None
            assert torch.equal(y.cpu(), w[i["start"]:i["end"]])
            continue
        assert abs(i["measured"] - want["measured"]) <= 0.01 and abs(i["gain"] / want["gain"] - 1) <= 1.2e-3
        if not i["limited"]:
            assert abs(L2 - -20.0) <= 0.01, L2                      # the output, measured again, is at the target
        else:
            assert L2 < -20.0 and float(y.abs().max()) <= 10 ** (-1 / 20) * (1 + 2.0 ** -23)
    assert sum(i["measured"] is None for i in info) == 1 and sum(i["start"] > 0 for i in info) >= 2
    assert sum(i["limited"] for i in info) >= 1 and sum(not i["limited"] and i["measured"] is not None for i in info) >= 1


def test_normalise_loudness_behind_kokoro_inference():
    _need_gpu()
    from kokoro.inference import normalise_loudness
    waves = [w.cuda() for w in _batch()]
    out, info = normalise_loudness(_norm(), waves, target_lufs=-30.0)
    want, winfo = _norm().normalise(waves, target_lufs=-30.0, peak_db=-1.0)
    assert info == winfo and all(torch.equal(a, b) for a, b in zip(out, want))
    assert [tuple(o.shape) for o in out] == [tuple(w.shape) for w in waves], "no trim: the lengths are kept"
    assert [i["limited"] for i in info] == [False, False, True, False] and info[1]["measured"] is None
    for L in _norm().measure([out[0], out[3]]):
        assert abs(L - -30.0) <= 0.01
    assert normalise_loudness(_norm(), []) == ([], [])


def test_value_errors():
    _need_gpu()
    from kokoro_ruslan_amd.loudness import LoudnessNormaliser
    n, w = _norm(), _batch()[1].cuda()
    for fs in (7999, 48001, 22050.5):
        with pytest.raises(ValueError, match="sample_rate"):
            LoudnessNormaliser(sample_rate=fs)
    for bad in (0.0, -40.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="top_db"):
            n.trim_edges([w], top_db=bad)
        with pytest.raises(ValueError, match="top_db"):
            n.normalise([w], trim_db=bad)
    for bad in (0.1, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="peak_db"):
            n.normalise([w], peak_db=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target_lufs"):
            n.normalise([w], target_lufs=bad)
    with pytest.raises(ValueError, match="margin_ms"):
        n.trim_edges([w], margin_ms=-1.0)
    with pytest.raises(ValueError, match="waveform 1"):
        n.measure([w, w[:0]])
    with pytest.raises(ValueError, match="waveform 0"):
        n.normalise([w.reshape(2, -1)])
    assert n.measure([]) == [] and n.trim_edges([]) == [] and n.normalise([]) == ([], [])


def test_kokoro_synth_with_loudness(tmp_path, capsys):
    """kokoro-synth --griffin-lim --loudness -20: every .wav read back measures -20 +- 0.05 LUFS (the int16 rounding) or is named as
    peak-limited in the summary line, and then peaks at the ceiling; without the flag the bytes are the peak-normalised ones."""
    _need_gpu()
    from kokoro.cli import synth as cli
    from kokoro.data.features import load_wav
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
    common = ["--checkpoint", str(ck), "--ids", str(ids_file), "--batch-size", "2", "--math", "f32", "--max-len", "60", "--min-len-floor",
              "45", "--weights", "model", "--griffin-lim", "--griffin-lim-iters", "5", "--griffin-lim-seed", "7"]
    plain, level = tmp_path / "plain", tmp_path / "level"
    assert cli.main(common + ["--output", str(plain)]) == 0
    plain_line = capsys.readouterr().out.strip().splitlines()[-1]
    assert cli.main(common + ["--output", str(level), "--loudness", "-20"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert "LUFS" not in plain_line and "-20 LUFS under -1 dB" in line
    limited = line.split("peak-limited: ")[1].split(",")[0].split(")")[0].split() if "peak-limited" in line else []
    assert "too short" not in line, line
    waves = [load_wav(str(level / f"{k}.wav")) for k in utts]
    assert all(w.numel() >= 44 * 256 for w in waves)
    for k, w, L in zip(utts, waves, _norm().measure(waves)):
        assert (plain / f"{k}.npy").read_bytes() == (level / f"{k}.npy").read_bytes()
        p = load_wav(str(plain / f"{k}.wav"))
        assert p.shape == w.shape and abs(float(p.abs().max()) - 32767 / 32768) < 1e-6, "without the flag: peak-normalised as before"
        print(f"{k}: {L:.4f} LUFS, peak {float(w.abs().max()):.4f}, limited {k in limited}")
        if k in limited:
            assert L < -20.0 and float(w.abs().max()) <= (10 ** (-1 / 20) * 32767 + 1) / 32768
        else:
            assert abs(L - -20.0) <= 0.05, (k, L)


def test_kokoro_precompute_conditions_the_corpus(tmp_path, capsys):
    _need_gpu()
    from scipy.io import wavfile
    from kokoro.cli import precompute as cli
    from kokoro.data.features import cache_path, load_wav
    wavs, cond, cache = tmp_path / "wavs", tmp_path / "cond", tmp_path / "cache"
    wavs.mkdir()
    shapes = {"a": (40000, 9000, 7000), "b": (30000, 0, 11000), "c": (52000, 15000, 2000)}
    lines, want = [], {}
    for i, (name, (n, lead, tail)) in enumerate(shapes.items()):
        x = _speechlike(n, 10 + i, 0.05 * (i + 1), lead, tail)
        wavfile.write(str(wavs / f"{name}.wav"), FS, np.rint(x.numpy() * 32767).astype(np.int16))
        lines.append({"name": name, "phoneme_indices": [3, 4, 5, 6]})
        y, info = LT.normalise(load_wav(str(wavs / f"{name}.wav")), -23.0, -1.0, trim=40.0)
        assert info["trim_margin"] >= 0.01 and info["gate_margin"] >= 0.01 and info["end"] - info["start"] < n - 2000
        want[name] = (y, info)
    ids = tmp_path / "u.jsonl"
    ids.write_text("".join(json.dumps(l) + "\n" for l in lines))
    argv = ["--wavs", str(wavs), "--ids", str(ids), "--batch-size", "2"]
    assert cli.main(argv + ["--cache-dir", str(tmp_path / "plain")]) == 0
    capsys.readouterr()
    assert cli.main(argv + ["--cache-dir", str(cache), "--trim-silence", "--loudness", "--conditioned-wavs", str(cond)]) == 0
    out = capsys.readouterr().out
    cut = sum(shapes[k][0] - (want[k][1]["end"] - want[k][1]["start"]) for k in shapes)
    summary = [l for l in out.splitlines() if "conditioning:" in l]
    assert len(summary) == 1 and f"{cut} samples trimmed" in summary[0] and "0 gains peak-limited" in summary[0], out
    for k, (n, _, _) in shapes.items():
        y, info = want[k]
        m = info["end"] - info["start"]
        entry = torch.load(cache_path(str(cache), k), map_location="cpu", weights_only=False)
        before = torch.load(cache_path(str(tmp_path / "plain"), k), map_location="cpu", weights_only=False)
        assert entry["mel_length"] == entry["pitch"].shape[0] == 1 + m // 256 < before["mel_length"] == 1 + n // 256
        assert entry["mel_spec"].numel() == 80 * entry["mel_length"]
        assert int(entry["phoneme_durations"].sum()) == entry["mel_length"]
        w = load_wav(str(cond / f"{k}.wav"))
        assert w.shape == (m,)
        assert float((w.double() * 32768 / 32767 - y).abs().max()) <= 1.2e-3 * float(y.abs().max()) + 1.0 / 32767
    lines[1]["phoneme_durations"] = [40, 40, 40, 38]
    ids.write_text("".join(json.dumps(l) + "\n" for l in lines))
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--cache-dir", str(tmp_path / "refused"), "--trim-silence"])
    assert e.value.code == 2 and "b carries phoneme_durations" in capsys.readouterr().err
    assert not (tmp_path / "refused").exists()
