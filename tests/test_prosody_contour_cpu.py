"""CPU suite: frame-level prosody contours.  The torch restatement of kk_prosody_contour (prosody_torch.contour) against the naive
per-frame loop of tests/prosody_contour_cases.py, the new fields of Prosody (validation, JSON, from_tracks), pack_contours, and the
command-line flags --oracle-prosody and --copy-prosody.  No GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prosody_contour_cases as CC  # noqa: E402
from kokoro_ruslan_amd import prosody_torch as PT  # noqa: E402
from kokoro_ruslan_amd.prosody import PackedContours, Prosody, pack, pack_contours  # noqa: E402

NAN = math.nan


def _equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# ---- the oracle against the definition ----------------------------------------------------------------------------------------

def _hand_case():
    """One row, phoneme by phoneme: 0 n = m (identity); 1 n = 3m; 2 m = 3n; 3 m = 0 with n > 0 (today's rule: forced 0.25); 4 n = 0;
    5 a NaN hole in the middle (today's rule there: the scaled prediction); 6 voiced values under scale 0.5 and shift 0.125;
    7 unvoiced values (0) under a shift; then two frames past lens."""
    dur = torch.tensor([[2, 6, 2, 3, 0, 3, 2, 2]])
    sd = torch.tensor([[2, 2, 6, 0, 2, 3, 2, 2]], dtype=torch.int32)
    pc = torch.tensor([[0.5, 0.25,  0.75, 0.125,  0.0625, 0.1875, 0.3125, 0.4375, 0.5625, 0.6875,  0.875, 0.875,  0.25, NAN, 0.75,  0.5, 1.0,  0.0, 0.0]])
    ec = torch.tensor([[0.5, 0.25,  0.75, 0.125,  0.0625, 0.1875, 0.3125, 0.4375, 0.5625, 0.6875,  0.875, 0.875,  0.25, NAN, 0.75,  0.5, 1.0,  0.5, 0.25]])
    T = 22
    idx, lens = CC.frames_of(dur, T)
    assert int(lens[0]) == 20
    g = torch.Generator().manual_seed(3)
    pitch, energy = torch.rand(1, T, generator=g) * 0.8 + 0.1, torch.rand(1, T, generator=g) * 0.8 + 0.1
    pitch[0, 21] = 1.5
    t = pack([Prosody(pitch_scale=[1, 1, 1, 1, 1, 2.0, 0.5, 1], pitch_shift=[0, 0, 0, 0, 0, 0, 0.125, 0.3],
                      energy_scale=[1, 1, 1, 1, 1, 1, 0.5, 2.0], energy_shift=[0, 0, 0, 0, 0, 0, 0, 0.25],
                      pitch=[NAN, NAN, NAN, 0.25, NAN, NAN, NAN, NAN])], [8], 8)
    return (pitch, energy, idx, lens, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy, dur, sd, pc, ec)


def test_contour_hand_case_frame_by_frame():
    args = _hand_case()
    pitch, energy = args[0], args[1]
    p, e = PT.contour(*args)
    want_p, want_e = CC.naive_contour(*args)
    assert _equal(p, want_p) and _equal(e, want_e)
    cp = pitch.clamp(0, 1)[0]
    got = p[0].tolist()
    assert got[0:2] == [0.5, 0.25], "n = m: the identity"
    assert got[2:8] == [0.75] * 3 + [0.125] * 3, "n = 3m: each source frame held over three frames"
    assert got[8:10] == [0.1875, 0.5625], "m = 3n: the centre of each third"
    assert got[10:13] == [0.25] * 3, "m = 0: the per-phoneme forced value"
    assert got[13] == 0.5 and got[15] == 1.0, "scale 2 on 0.25 and on 0.75, clamped"
    assert got[14] == float((cp[14] * 2.0).clamp(0, 1)), "a NaN hole: the scaled prediction"
    assert got[16:18] == [0.375, 0.625], "a voiced value is scaled, then shifted"
    assert got[18:20] == [0.0, 0.0], "an unvoiced source frame stays unvoiced under any shift"
    assert got[20] == float(cp[20]) and got[21] == 1.0, "past lens: the clamped prediction"
    ge = e[0].tolist()
    assert ge[16:18] == [0.25, 0.5] and ge[18:20] == [1.0, 0.75], "energy: scaled and shifted, clamped"
    assert ge[10:13] == energy[0, 10:13].tolist(), "m = 0, nothing forced, neutral tables: the prediction"


@pytest.mark.parametrize("Pn", [1, 5, 70])
def test_contour_equals_the_naive_loop_on_the_kernel_tests_inputs(Pn):
    args = CC.kernel_inputs(Pn, 40 + Pn)
    p, e = PT.contour(*args)
    want_p, want_e = CC.naive_contour(*args)
    assert _equal(p, want_p) and _equal(e, want_e)
    p1, e1 = PT.contour(*args[:12], args[12], None)                # no energy track in the batch
    v_p, v_e = PT.variance(*args[:10])
    assert _equal(p1, want_p) and _equal(e1, v_e)
    if Pn > 1:
        assert not _equal(p, v_p) and not _equal(e, v_e), "the contours act"


def test_a_row_without_a_contour_equals_variance():
    args = CC.kernel_inputs(70, 9)
    p, e = PT.contour(*args)
    v_p, v_e = PT.variance(*args[:10])
    assert torch.equal(p[0], v_p[0]) and torch.equal(e[0], v_e[0]), "row 0: sd = 0"
    assert torch.equal(e[1], v_e[1]), "row 1: a pitch track only"
    nan = torch.full_like(args[12], NAN)
    p, e = PT.contour(*args[:12], nan, nan)
    assert torch.equal(p, v_p) and torch.equal(e, v_e), "tracks of NaN"
    p, e = PT.contour(*args[:11], torch.zeros_like(args[11]), args[12], args[13])
    assert torch.equal(p, v_p) and torch.equal(e, v_e), "no source frames"
    p, e = PT.contour(*args[:12], None, None)
    assert torch.equal(p, v_p) and torch.equal(e, v_e), "no tracks"


# ---- Prosody: validation ----------------------------------------------------------------------------------------------------------

def test_validate_accepts_contours():
    Prosody(pitch_contour=[0.0, NAN, 1.0, 0.5], contour_durations=[1, 0, 3]).validate(3)
    Prosody(energy_contour=[0.5] * 4, pitch_contour=[NAN] * 4, contour_durations=[4, 0, 0]).validate(3)
    Prosody(durations=[2, 0, 2], pitch_contour=[0.5] * 4).validate(3)                  # contour_durations = durations
    Prosody(durations=[-1, 5, 2], pitch_contour=[0.5] * 4, contour_durations=[2, 1, 1]).validate(3)
    Prosody(pitch_contour=[0.5] * 4096, contour_durations=[4096, 0, 0]).validate(3)
    Prosody(pitch_contour=[], contour_durations=[0, 0, 0]).validate(3)


@pytest.mark.parametrize("kw,what", [
    ({"pitch_contour": [0.5] * 4, "energy_contour": [0.5] * 5, "contour_durations": [2, 1, 1]}, "differ in length"),
    ({"pitch_contour": [0.5] * 4, "contour_durations": [2, 1, 2]}, "sum to 5"),
    ({"durations": [2, 1, 2], "energy_contour": [0.5] * 4}, "sum to 5"),
    ({"pitch_contour": [0.5, 1.5, 0.5, 0.5], "contour_durations": [2, 1, 1]}, "pitch_contour must be in"),
    ({"energy_contour": [0.5, -0.1, 0.5, 0.5], "contour_durations": [2, 1, 1]}, "energy_contour must be in"),
    ({"pitch_contour": [0.5, math.inf, 0.5, 0.5], "contour_durations": [2, 1, 1]}, "pitch_contour must be in"),
    ({"pitch_contour": [0.5] * 4097, "contour_durations": [4097, 0, 0]}, "4096"),
    ({"pitch_contour": [0.5] * 4, "durations": [2, -1, 2]}, "contour_durations"),
    ({"pitch_contour": [0.5] * 4}, "contour_durations"),
    ({"pitch_contour": [0.5] * 4, "contour_durations": [2, 2]}, "contour_durations"),
    ({"pitch_contour": [0.5] * 4, "contour_durations": [5, -1, 0]}, "contour_durations must be >= 0"),
    ({"pitch_contour": 0.5, "contour_durations": [1, 0, 0]}, "pitch_contour"),
    ({"contour_durations": [1, 1, 1]}, "without"),
    ({"pitch_contour": [0.5] * 3, "contour_durations": [1.5, 0.5, 1]}, "contour_durations")])
def test_validate_rejects_contours(kw, what):
    with pytest.raises(ValueError, match=what):
        Prosody(**kw).validate(3)


def test_is_neutral_accounts_for_contours():
    assert Prosody(pitch_contour=[NAN, NAN], energy_contour=[NAN, NAN], contour_durations=[1, 1]).is_neutral()
    assert not Prosody(pitch_contour=[NAN, 0.0], contour_durations=[1, 1]).is_neutral()
    assert not Prosody(energy_contour=[0.5, NAN], contour_durations=[1, 1]).is_neutral()


# ---- Prosody: round trips ---------------------------------------------------------------------------------------------------------

def test_from_json_takes_contours_with_nulls():
    p = Prosody.from_json({"pitch_contour": [0.5, None, 0.25], "energy_contour": [None, None, 1.0], "contour_durations": [2, 1],
                           "pitch_shift": 0.1}, 2)
    assert p.pitch_contour[0] == 0.5 and math.isnan(p.pitch_contour[1]) and p.pitch_contour[2] == 0.25
    assert math.isnan(p.energy_contour[0]) and p.energy_contour[2] == 1.0 and p.contour_durations == [2, 1] and p.pitch_shift == 0.1
    with pytest.raises(ValueError, match="sum to 3"):
        Prosody.from_json({"pitch_contour": [0.5, None], "contour_durations": [2, 1]}, 2)
    with pytest.raises(ValueError, match="pitch_contour"):
        Prosody.from_json({"pitch_contour": 0.5, "contour_durations": [2, 1]}, 2)
    with pytest.raises(ValueError, match="contour_durations"):
        Prosody.from_json({"pitch_contour": [0.5], "contour_durations": 1}, 2)
    with pytest.raises(ValueError, match="numbers"):
        Prosody.from_json({"pitch_contour": ["a"], "contour_durations": [1, 0]}, 2)
    assert Prosody.from_json({"durations": [1, 2], "energy_contour": [0.1, 0.2, None]}, 2).contours(2)[2].tolist() == [1, 2]


def test_from_tracks_cuts_and_pads():
    dur = torch.tensor([2, 0, 3])
    p = Prosody.from_tracks(dur, torch.arange(8) / 8.0, torch.tensor([0.5, 0.25, 1.0])).validate(3)
    assert p.durations.tolist() == [2, 0, 3] and p.contour_durations.tolist() == [2, 0, 3]
    assert p.pitch_contour.tolist() == [0.0, 0.125, 0.25, 0.375, 0.5], "a longer track is cut at sum(durations)"
    assert p.energy_contour[:3].tolist() == [0.5, 0.25, 1.0] and bool(torch.isnan(p.energy_contour[3:]).all()) and p.energy_contour.numel() == 5
    q = Prosody.from_tracks([2, 0, 3], [0.5] * 5, None, force_durations=False, pitch_shift=0.1).validate(3)
    assert q.durations is None and q.energy_contour is None and q.contour_durations.tolist() == [2, 0, 3] and q.pitch_shift == 0.1
    r = Prosody.from_tracks([2, 0, 3]).validate(3)
    assert r.pitch_contour is None and r.contour_durations is None and r.durations.tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        Prosody.from_tracks([2, -1, 3], [0.5] * 5)


# ---- pack_contours ----------------------------------------------------------------------------------------------------------------

def test_pack_contours():
    assert pack_contours(None, [3, 2], 3) is None
    assert pack_contours([None, Prosody(speed=2.0, pitch=[0.5, NAN])], [3, 2], 3) is None
    assert pack_contours([Prosody(pitch_contour=[], contour_durations=[0, 0, 0]), None], [3, 2], 3) is None
    rows = [Prosody(pitch_contour=[0.5, NAN, 0.25, 0.0], contour_durations=[1, 0, 3]), None,
            Prosody(durations=[1, 1], pitch_contour=[0.1, 0.2], energy_contour=[0.3, NAN])]
    c = pack_contours(rows, [3, 1, 2], 4)
    assert isinstance(c, PackedContours) and c.pitch.shape == (3, 4) and c.energy.shape == (3, 4) and c.src_dur.shape == (3, 4)
    assert c.src_dur.dtype == torch.int32 and c.src_dur.tolist() == [[1, 0, 3, 0], [0, 0, 0, 0], [1, 1, 0, 0]]
    assert c.pitch.dtype == torch.float32 and c.pitch[0, [0, 2, 3]].tolist() == [0.5, 0.25, 0.0] and math.isnan(float(c.pitch[0, 1]))
    assert bool(torch.isnan(c.pitch[1]).all()) and bool(torch.isnan(c.energy[:2]).all()), "rows without a track carry NaN"
    assert c.pitch[2, :2].tolist() == [torch.tensor(0.1).item(), torch.tensor(0.2).item()] and bool(torch.isnan(c.pitch[2, 2:]).all())
    assert float(c.energy[2, 0]) == torch.tensor(0.3).item() and bool(torch.isnan(c.energy[2, 1:]).all())
    assert pack_contours(rows[:2], [3, 1], 3).energy is None, "no energy track in the batch: a null pointer for the kernel"
    with pytest.raises(ValueError, match="utterance 0"):
        pack_contours(rows, [2, 1, 2], 4)
    with pytest.raises(ValueError, match="4097 phonemes"):
        pack_contours([Prosody(pitch_contour=[0.5], contour_durations=[1] + [0] * 4096)], [4097], 4097)
    with pytest.raises(ValueError, match="4096"):
        pack_contours([Prosody(pitch_contour=[0.5] * 4097, contour_durations=[4097])], [1], 1)


# ---- the command-line surface -----------------------------------------------------------------------------------------------------

EVAL = ["--checkpoint", "c", "--features", "d"]
SYNTH = ["--checkpoint", "c", "--output", "o"]


def test_eval_oracle_prosody_implies_oracle_durations():
    from kokoro.cli import evaluate as cli
    p = cli.build_parser()
    a = p.parse_args(EVAL)
    cli.check_args(p, a)
    assert not hasattr(a, "oracle_prosody") and a.oracle_durations is False, "not given: the namespace is as before"
    b = p.parse_args(EVAL + ["--oracle-durations"])
    cli.check_args(p, b)
    assert not hasattr(b, "oracle_prosody") and b.oracle_durations is True
    c = p.parse_args(EVAL + ["--oracle-prosody"])
    cli.check_args(p, c)
    assert c.oracle_prosody is True and c.oracle_durations is True
    assert {k: v for k, v in vars(c).items() if k != "oracle_prosody"} == vars(b)


def test_eval_oracle_prosody_builds_the_controls_and_names_what_is_missing():
    from kokoro.cli import evaluate as cli
    ids = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    durs = [torch.tensor([2, 0, 3]), torch.tensor([1, 2])]
    pitch = [torch.tensor([0.5, 0.0, 0.25, 0.125, 1.0, 0.75]), torch.tensor([0.5, 0.25])]        # one frame more, one fewer
    energy = [torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]), torch.tensor([0.5, 0.25])]
    a, b = cli.oracle_prosody(["a", "b"], ids, durs, pitch, energy)
    assert a.durations.tolist() == [2, 0, 3] and a.pitch_contour.tolist() == [0.5, 0.0, 0.25, 0.125, 1.0]
    assert b.energy_contour[:2].tolist() == [0.5, 0.25] and math.isnan(float(b.energy_contour[2])) and b.contour_durations.tolist() == [1, 2]
    only = cli.oracle_prosody(["a", "b"], ids, durs)
    assert only[0].pitch_contour is None and only[0].durations.tolist() == [2, 0, 3]
    with pytest.raises(ValueError, match="--oracle-prosody: utterance b has no pitch and energy"):
        cli.oracle_prosody(["a", "b"], ids, durs, [pitch[0], torch.zeros(3)], [energy[0], torch.zeros(3)])
    with pytest.raises(ValueError, match="--oracle-prosody: utterance a has no durations"):
        cli.oracle_prosody(["a", "b"], ids, [torch.tensor([1, 2]), durs[1]], pitch, energy)


def test_synth_copy_prosody_flag():
    from kokoro.cli import synth as cli
    p = cli.build_parser()
    a = p.parse_args(SYNTH + ["--features", "d"])
    cli.check_args(p, a)
    assert not hasattr(a, "copy_prosody") and cli.copy_parts(a) == (), "not given: the namespace is as before"
    a = p.parse_args(SYNTH + ["--features", "d", "--copy-prosody"])
    cli.check_args(p, a)
    assert cli.copy_parts(a) == ("durations", "pitch", "energy")
    a = p.parse_args(SYNTH + ["--features", "d", "--copy-prosody", "energy", "pitch", "--pitch-shift", "0.1"])
    cli.check_args(p, a)
    assert cli.copy_parts(a) == ("pitch", "energy") and cli.prosody_flags(a) == {"pitch_shift": 0.1}


@pytest.mark.parametrize("argv", [SYNTH + ["--ids", "u.jsonl", "--copy-prosody"], SYNTH + ["--features", "d", "--copy-prosody", "speed"]])
def test_synth_copy_prosody_errors(argv, capsys):
    from kokoro.cli import synth as cli
    p = cli.build_parser()
    with pytest.raises(SystemExit) as ex:
        cli.check_args(p, p.parse_args(argv))
    assert ex.value.code == 2 and "--copy-prosody" in capsys.readouterr().err


def test_synth_copied_prosody():
    from kokoro.cli import synth as cli
    ids, durs = [torch.tensor([1, 2, 3])], [torch.tensor([2, 0, 3])]
    pitch, energy = [torch.tensor([0.5, 0.0, 0.25, 0.125, 1.0, 0.75])], [torch.tensor([0.1, 0.2, 0.3])]
    (pr,) = cli.copied_prosody(["a"], ids, durs, pitch, energy, ("durations", "pitch", "energy"), {"pitch_shift": 0.1})
    assert pr.durations.tolist() == [2, 0, 3] and pr.pitch_contour.numel() == 5 and pr.energy_contour.numel() == 5 and pr.pitch_shift == 0.1
    (pr,) = cli.copied_prosody(["a"], ids, durs, pitch, energy, ("pitch",), {})
    assert pr.durations is None and pr.energy_contour is None and pr.contour_durations.tolist() == [2, 0, 3]
    (pr,) = cli.copied_prosody(["a"], ids, durs, pitch, energy, ("durations",), {})
    assert pr.durations.tolist() == [2, 0, 3] and pr.pitch_contour is None and pr.contour_durations is None
    with pytest.raises(ValueError, match="utterance a has no energy"):
        cli.copied_prosody(["a"], ids, durs, pitch, [torch.zeros(5)], ("energy",), {})
    with pytest.raises(ValueError, match="utterance a has no durations"):
        cli.copied_prosody(["a"], ids, [torch.tensor([1, 2])], pitch, energy, ("pitch",), {})


def test_ids_line_carries_a_contour(tmp_path):
    from kokoro.cli import synth as cli
    f = tmp_path / "u.jsonl"
    f.write_text('{"name": "a", "phoneme_indices": [1, 2], "prosody": {"pitch_contour": [0.5, null, 0.25], "contour_durations": [1, 2]}}\n')
    (pr,) = cli.read_prosody(str(f), {"pitch_shift": 0.05})
    assert pr.pitch_shift == 0.05 and math.isnan(pr.pitch_contour[1]) and pr.contour_durations == [1, 2]
    f.write_text('{"name": "a", "phoneme_indices": [1, 2], "prosody": {"pitch_contour": [0.5, 0.25], "contour_durations": [1, 2]}}\n')
    with pytest.raises(ValueError, match="u.jsonl:1"):
        cli.read_prosody(str(f), {})
