"""The loudness and trimming flags of kokoro-synth and kokoro-precompute at the parser: defaults, refusals, and that an invocation
without them parses every earlier option to the value it had before the flags existed.  No GPU."""
import pytest

from kokoro.cli import precompute as pre
from kokoro.cli import synth

SYNTH = ["--checkpoint", "ck", "--ids", "u.jsonl", "--output", "out"]
PRE = ["--wavs", "w", "--ids", "u.jsonl", "--cache-dir", "c"]
# every option of the two parsers before the loudness flags, at its default
SYNTH_BEFORE = {"checkpoint": "ck", "features": None, "ids": "u.jsonl", "indices": None, "output": "out", "batch_size": 32,
                "weights": "auto", "stop_threshold": None, "max_len": None, "min_len_ratio": None, "min_len_floor": None, "trim": False,
                "math": "bf16", "stream": False, "slots": None, "vocoder": None, "vocoder_config": None, "vocoder_math": "bf16",
                "denoise": None, "griffin_lim": False, "griffin_lim_iters": 60, "griffin_lim_seed": None}
PRE_BEFORE = {"wavs": "w", "ids": "u.jsonl", "cache_dir": "c", "force": False, "no_variance": False, "resample": False, "batch_size": 32,
              "max_seq_length": 1800, "n_mels": 80, "hop_length": 256, "sample_rate": 22050}


def _parse(mod, argv):
    p = mod.build_parser()
    args = p.parse_args(argv)
    mod.check_args(p, args)
    return args


def _refused(mod, argv, capsys, match):
    with pytest.raises(SystemExit) as e:
        _parse(mod, argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def test_synth_defaults_and_values():
    a = _parse(synth, SYNTH)
    assert a.loudness is None and a.peak_db == -1.0
    a = _parse(synth, SYNTH + ["--griffin-lim", "--loudness"])
    assert a.loudness == -23.0 and a.peak_db == -1.0
    a = _parse(synth, SYNTH + ["--vocoder", "v", "--denoise", "--loudness", "-16", "--peak-db", "-2.5"])
    assert a.loudness == -16.0 and a.peak_db == -2.5 and a.denoise == 0.005


def test_synth_refusals(capsys):
    _refused(synth, SYNTH + ["--loudness"], capsys, "--loudness needs --vocoder or --griffin-lim")
    _refused(synth, SYNTH + ["--loudness", "-20"], capsys, "--loudness needs --vocoder or --griffin-lim")
    _refused(synth, SYNTH + ["--griffin-lim", "--peak-db", "-3"], capsys, "--peak-db needs --loudness")
    _refused(synth, SYNTH + ["--griffin-lim", "--loudness", "--peak-db", "1"], capsys, "--peak-db must be <= 0")
    _refused(synth, SYNTH + ["--griffin-lim", "--loudness", "nan"], capsys, "--loudness must be finite")


def test_precompute_defaults_and_values():
    a = _parse(pre, PRE)
    assert a.trim_silence is None and a.loudness is None and a.peak_db == -1.0 and a.conditioned_wavs is None
    a = _parse(pre, PRE + ["--trim-silence", "--loudness", "--conditioned-wavs", "d"])
    assert a.trim_silence == 40.0 and a.loudness == -23.0 and a.conditioned_wavs == "d"
    a = _parse(pre, PRE + ["--trim-silence", "35", "--loudness", "-20", "--peak-db", "-3"])
    assert (a.trim_silence, a.loudness, a.peak_db) == (35.0, -20.0, -3.0)
    assert "kokoro-align" in pre.build_parser().format_help()


def test_precompute_refusals(capsys):
    _refused(pre, PRE + ["--trim-silence", "0"], capsys, "--trim-silence must be > 0")
    _refused(pre, PRE + ["--trim-silence", "-40"], capsys, "--trim-silence must be > 0")
    _refused(pre, PRE + ["--loudness", "inf"], capsys, "--loudness must be finite")
    _refused(pre, PRE + ["--loudness", "--peak-db", "0.5"], capsys, "--peak-db must be <= 0")
    _refused(pre, PRE + ["--peak-db", "-3"], capsys, "--peak-db needs --loudness")
    _refused(pre, PRE + ["--conditioned-wavs", "d"], capsys, "--conditioned-wavs needs --trim-silence or --loudness")


def test_trim_silence_refuses_given_durations_before_any_device_work(tmp_path, capsys):
    import json
    ids = tmp_path / "u.jsonl"
    ids.write_text(json.dumps({"name": "a", "phoneme_indices": [1, 2]}) + "\n"
                   + json.dumps({"name": "b", "phoneme_indices": [1, 2], "phoneme_durations": [3, 4]}) + "\n")
    with pytest.raises(SystemExit) as e:
        pre.main(["--wavs", str(tmp_path), "--ids", str(ids), "--cache-dir", str(tmp_path / "c"), "--trim-silence"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "b carries phoneme_durations" in err and "kokoro-align" in err
    assert not (tmp_path / "c").exists()


def test_invocations_without_the_flags_parse_as_before():
    a = vars(_parse(synth, SYNTH))
    assert {k: a[k] for k in SYNTH_BEFORE} == SYNTH_BEFORE
    assert set(a) - set(SYNTH_BEFORE) == {"loudness", "peak_db"}
    a = vars(_parse(synth, SYNTH + ["--vocoder", "v", "--denoise", "0.01", "--batch-size", "4", "--trim"]))
    assert {k: a[k] for k in SYNTH_BEFORE} == dict(SYNTH_BEFORE, vocoder="v", denoise=0.01, batch_size=4, trim=True)
    a = vars(_parse(pre, PRE))
    assert {k: a[k] for k in PRE_BEFORE} == PRE_BEFORE
    assert set(a) - set(PRE_BEFORE) == {"trim_silence", "loudness", "peak_db", "conditioned_wavs"}
    a = vars(_parse(pre, PRE + ["--resample", "--force", "--max-seq-length", "900"]))
    assert {k: a[k] for k in PRE_BEFORE} == dict(PRE_BEFORE, resample=True, force=True, max_seq_length=900)
