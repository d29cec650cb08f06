"""CPU suite: the prosody controls' public type (validation, JSON, packing), the algebra of the torch restatement of the two kernels,
and the command-line surface.  No GPU."""
import json
import math

import pytest
import torch

from kokoro_ruslan_amd import prosody_torch as PT
from kokoro_ruslan_amd.prosody import PackedProsody, Prosody, as_list, pack

NAN = math.nan


# ---- Prosody.validate -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    {}, {"speed": 0.25}, {"speed": 4.0}, {"speed": [1.0, 2.0, 0.5]}, {"speed": torch.tensor([1.0, 2.0, 0.5])},
    {"pitch_scale": 0.0}, {"pitch_scale": [0.5, 1.0, 2.0]}, {"pitch_shift": -0.3}, {"pitch_shift": [0.1, -0.1, 0.0]},
    {"energy_scale": 3.0}, {"energy_scale": [1.0, 0.0, 1.5]}, {"energy_shift": 0.2}, {"energy_shift": [0.0, 0.5, -0.5]},
    {"durations": [0, -1, 7]}, {"durations": torch.tensor([3, 3, 3])}, {"pitch": [0.0, NAN, 1.0]}, {"energy": [NAN, 0.5, NAN]},
    {"speed": 2, "durations": [1, 1, 1], "pitch": [0.5, 0.5, 0.5], "energy": [0.5, 0.5, 0.5]}])
def test_validate_accepts(kw):
    p = Prosody(**kw)
    assert p.validate(3) is p


@pytest.mark.parametrize("kw,what", [
    ({"speed": [1.0, 1.0]}, "speed"), ({"pitch_scale": [1.0] * 4}, "pitch_scale"), ({"pitch_shift": [0.0] * 2}, "pitch_shift"),
    ({"energy_scale": [1.0] * 2}, "energy_scale"), ({"energy_shift": [0.0] * 4}, "energy_shift"),
    ({"durations": [1, 2]}, "durations"), ({"pitch": [0.5] * 4}, "pitch"), ({"energy": [0.5] * 2}, "energy"),
    ({"durations": 3}, "durations"), ({"pitch": 0.5}, "pitch"),
    ({"speed": 0.2}, "speed"), ({"speed": 4.5}, "speed"), ({"speed": [1.0, 0.1, 1.0]}, "speed"), ({"speed": NAN}, "speed"),
    ({"pitch_scale": -0.1}, "pitch_scale"), ({"energy_scale": [1.0, -1.0, 1.0]}, "energy_scale"),
    ({"pitch_scale": math.inf}, "pitch_scale"),
    ({"pitch_shift": math.inf}, "pitch_shift"), ({"energy_shift": NAN}, "energy_shift"), ({"pitch_shift": [0.0, NAN, 0.0]}, "pitch_shift"),
    ({"durations": [1, -2, 1]}, "durations"), ({"durations": [1.5, 1, 1]}, "durations"),
    ({"pitch": [0.5, 1.1, 0.5]}, "pitch"), ({"pitch": [-0.1, 0.5, 0.5]}, "pitch"), ({"energy": [0.5, 0.5, 2.0]}, "energy"),
    ({"energy": [0.5, -math.inf, 0.5]}, "energy"), ({"speed": "fast"}, "speed"), ({"speed": None}, "speed")])
def test_validate_rejects(kw, what):
    with pytest.raises(ValueError, match=what):
        Prosody(**kw).validate(3)


def test_is_neutral():
    assert Prosody().is_neutral()
    assert Prosody(speed=[1.0, 1.0], pitch_scale=1, energy_shift=[0.0, 0.0], durations=[-1, -1], pitch=[NAN, NAN], energy=[NAN, NAN]).is_neutral()
    for kw in ({"speed": 1.1}, {"speed": [1.0, 2.0]}, {"pitch_scale": 0.9}, {"pitch_shift": 0.1}, {"energy_scale": 2.0},
               {"energy_shift": [0.0, -0.1]}, {"durations": [-1, 0]}, {"pitch": [NAN, 0.0]}, {"energy": [1.0, NAN]}):
        assert not Prosody(**kw).is_neutral(), kw


# ---- Prosody.from_json ----------------------------------------------------------------------------------------------------------

def test_from_json_accepts_scalars_lists_and_nulls():
    p = Prosody.from_json({"speed": 1.5, "pitch_scale": [1.0, 2.0], "energy_shift": -0.25, "durations": [4, -1], "pitch": [None, 0.25],
                           "energy": [0.5, NAN], "pitch_shift": None}, 2)
    assert p.speed == 1.5 and p.pitch_scale == [1.0, 2.0] and p.energy_shift == -0.25 and p.durations == [4, -1]
    assert math.isnan(p.pitch[0]) and p.pitch[1] == 0.25 and p.energy[0] == 0.5 and math.isnan(p.energy[1])
    assert p.pitch_shift == 0.0, "null leaves the field at its neutral value"
    assert Prosody.from_json({}, 5).is_neutral()
    assert Prosody.from_json(json.loads('{"speed": 2, "durations": [1, 2, 3]}'), 3).durations == [1, 2, 3]


@pytest.mark.parametrize("obj", [
    {"tempo": 1.0}, {"speed": 5.0}, {"speed": "2"}, {"speed": True}, {"durations": 3}, {"durations": [1, 2]}, {"pitch": 0.5},
    {"pitch": [0.5, 0.5, 7.0]}, {"energy": [0.5, "x", 0.5]}, {"pitch_scale": [1.0, 1.0]}, {"energy_scale": -1}, [1.0], "speed"])
def test_from_json_rejects(obj):
    with pytest.raises(ValueError):
        Prosody.from_json(obj, 3)


# ---- pack -----------------------------------------------------------------------------------------------------------------------

def test_pack_layout_and_neutral_padding():
    rows = [Prosody(speed=2.0, pitch_scale=[0.5, 1.5], pitch_shift=0.1, energy_scale=0.0, energy_shift=[0.2, -0.2], durations=[3, -1],
                    pitch=[NAN, 0.75], energy=[0.25, NAN]),
            None,
            Prosody(speed=[1.0, 0.5, 4.0, 0.25])]
    t = pack(rows, [2, 3, 4], 5)
    assert isinstance(t, PackedProsody)
    assert [tuple(x.shape) for x in t] == [(3, 5), (2, 3, 5), (2, 3, 5), (3, 5), (3, 5), (3, 5)]
    assert [x.dtype for x in t] == [torch.float32] * 5 + [torch.int32] and all(x.is_contiguous() for x in t)
    assert t.speed.tolist() == [[2, 2, 1, 1, 1], [1] * 5, [1, 0.5, 4, 0.25, 1]]
    assert torch.equal(t.pitch_ss[0], torch.tensor([[0.5, 1.5, 1, 1, 1], [1.0] * 5, [1.0] * 5]))
    assert torch.equal(t.pitch_ss[1], torch.tensor([[0.1, 0.1, 0, 0, 0], [0.0] * 5, [0.0] * 5]))
    assert torch.equal(t.energy_ss[0], torch.tensor([[0.0, 0, 1, 1, 1], [1.0] * 5, [1.0] * 5]))
    assert torch.equal(t.energy_ss[1], torch.tensor([[0.2, -0.2, 0, 0, 0], [0.0] * 5, [0.0] * 5]))
    assert t.durations.tolist() == [[3, -1, -1, -1, -1], [-1] * 5, [-1] * 5]
    assert bool(torch.isnan(t.pitch).sum() == 14) and float(t.pitch[0, 1]) == 0.75
    assert bool(torch.isnan(t.energy).sum() == 14) and float(t.energy[0, 0]) == 0.25
    neutral = pack([Prosody()] * 2, [1, 4], 4)
    for a, b in zip(neutral, pack([None, None], [1, 4], 4)):
        assert torch.equal(a, b) or bool(torch.isnan(a).all() and torch.isnan(b).all())


def test_pack_and_as_list_errors():
    with pytest.raises(ValueError, match="utterance 1"):
        pack([Prosody(), Prosody(speed=[1.0, 1.0])], [2, 3], 3)
    with pytest.raises(ValueError):
        pack([Prosody()], [2, 3], 3)
    with pytest.raises(ValueError):
        pack([Prosody()], [4], 3)
    with pytest.raises(ValueError):
        pack([{"speed": 1.0}], [3], 3)
    assert as_list(None, 3) is None
    p = Prosody(speed=2.0)
    assert as_list(p, 3) == [p, p, p] and as_list([p, None], 2) == [p, None]
    with pytest.raises(ValueError):
        as_list([p], 2)


# ---- the torch restatement's algebra ----------------------------------------------------------------------------------------------

def _neutral(B, Pn):
    t = pack([None] * B, [Pn] * B, Pn)
    return t


def test_durations_neutral_is_clamp_round():
    g = torch.Generator().manual_seed(0)
    d = torch.cat([torch.randn(4, 50, generator=g) * 6, torch.tensor([[0.5, 1.5, 2.5, -0.5, 0.49999997, 0.0, -3.0, 7.0]]).repeat(4, 1)], dim=1)
    t = _neutral(4, d.shape[1])
    dur, sums = PT.durations(d, t.speed, t.durations)
    want = torch.clamp(torch.round(d), min=0).to(torch.int64)
    assert dur.dtype == torch.int64 and torch.equal(dur, want) and torch.equal(sums, want.sum(dim=1))
    assert dur[0, -8:].tolist() == [0, 2, 2, 0, 0, 0, 0, 7], "half to even"


def test_durations_speed_min_one_frame_and_zero_stays_zero():
    d = torch.tensor([[0.4, 0.6, 1.0, 5.0, 9.0, -2.0, 2.5, 10.0]])
    none = torch.full((1, 8), -1, dtype=torch.int32)
    fast, _ = PT.durations(d, torch.full((1, 8), 4.0), none)
    assert fast.tolist() == [[0, 1, 1, 1, 2, 0, 1, 2]], "a phoneme with a frame keeps one; one without stays at 0; 2.5 -> half to even"
    slow, s = PT.durations(d, torch.full((1, 8), 0.25), none)
    assert slow.tolist() == [[0, 2, 4, 20, 36, 0, 10, 40]] and s.tolist() == [112]
    per, _ = PT.durations(d, torch.tensor([[1.0, 1.0, 0.5, 2.0, 4.0, 1.0, 1.0, 0.25]]), none)
    assert per.tolist() == [[0, 1, 2, 2, 2, 0, 2, 40]]


def test_durations_forced_wins_and_row_lengths():
    d = torch.tensor([[3.0, 0.2, 8.0, 1.0], [2.0, 2.0, 2.0, 2.0]])
    forced = torch.tensor([[-1, 5, 0, -1], [7, -1, -1, 9]], dtype=torch.int32)
    dur, sums = PT.durations(d, torch.full((2, 4), 2.0), forced)
    assert dur.tolist() == [[2, 5, 0, 1], [7, 1, 1, 9]] and sums.tolist() == [8, 18]
    dur, sums = PT.durations(d, torch.full((2, 4), 2.0), forced, plens=torch.tensor([2, 3], dtype=torch.int32))
    assert dur.tolist() == [[2, 5, 0, 0], [7, 1, 1, 0]] and sums.tolist() == [7, 9], "positions past the row's phonemes give 0"


def _var_case():
    pitch = torch.tensor([[-0.2, 0.0, 0.3, 0.6, 1.0, 1.4, 0.5, 0.5]])
    energy = torch.tensor([[0.1, -0.5, 0.4, 0.8, 1.2, 0.0, 0.5, 0.5]])
    idx = torch.tensor([[0, 0, 1, 1, 2, 2, -1, -1]])
    lens = torch.tensor([6])
    return pitch, energy, idx, lens


def test_variance_neutral_is_clamp():
    pitch, energy, idx, lens = _var_case()
    t = _neutral(1, 3)
    p, e = PT.variance(pitch, energy, idx, lens, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy)
    assert torch.equal(p, pitch.clamp(0, 1)) and torch.equal(e, energy.clamp(0, 1))


def test_variance_scale_shift_forced_and_unvoiced():
    pitch, energy, idx, lens = _var_case()
    t = pack([Prosody(pitch_scale=[2.0, 0.5, 1.0], pitch_shift=[0.1, 0.0, -0.25], energy_scale=[0.5, 2.0, 1.0], energy_shift=[0.25, 0.0, 0.5],
                      pitch=[NAN, NAN, 0.125], energy=[NAN, 0.75, NAN])], [3], 3)
    p, e = PT.variance(pitch, energy, idx, lens, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy)
    # phoneme 0: both of its frames are unvoiced (clamped pitch 0) and stay so whatever the shift; phoneme 1 scaled; phoneme 2 forced;
    # frames past lens keep the clamped prediction
    assert p.tolist() == [[0.0, 0.0, 0.15000000596046448, 0.30000001192092896, 0.125, 0.125, 0.5, 0.5]]
    assert e.tolist() == [[0.30000001192092896, 0.25, 0.75, 0.75, 1.0, 0.5, 0.5, 0.5]]
    # the results are clamped to [0, 1]
    t = pack([Prosody(pitch_scale=3.0, energy_shift=-0.6)], [3], 3)
    p, e = PT.variance(pitch, energy, idx, lens, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy)
    assert float(p.max()) == 1.0 and float(e.min()) == 0.0 and p[0, :2].tolist() == [0.0, 0.0]
    assert float(p[0, 2]) == float(torch.tensor(0.3) * torch.tensor(3.0)), "one fp32 product, then one fp32 sum"


# ---- the command-line surface ---------------------------------------------------------------------------------------------------

BASE = ["--checkpoint", "c", "--ids", "u.jsonl", "--output", "o"]


def test_synth_cli_flags_parse():
    from kokoro.cli import synth as cli
    p = cli.build_parser()
    a = p.parse_args(BASE)
    cli.check_args(p, a)
    assert not any(hasattr(a, k) for k in cli.PROSODY_FLAGS) and cli.prosody_flags(a) == {}, "not given: the namespace is as before"
    a = p.parse_args(BASE + ["--speed", "1.25", "--pitch-scale", "1.1", "--pitch-shift", "-0.05", "--energy-scale", "0.9", "--energy-shift", "0.1"])
    cli.check_args(p, a)
    assert cli.prosody_flags(a) == {"speed": 1.25, "pitch_scale": 1.1, "pitch_shift": -0.05, "energy_scale": 0.9, "energy_shift": 0.1}


@pytest.mark.parametrize("extra", [["--speed", "0.1"], ["--speed", "5"], ["--pitch-scale", "-1"], ["--energy-scale", "-0.5"],
                                   ["--pitch-shift", "nan"], ["--energy-shift", "inf"], ["--speed", "nan"]])
def test_synth_cli_flag_errors_go_through_parser_error(extra, capsys):
    from kokoro.cli import synth as cli
    p = cli.build_parser()
    with pytest.raises(SystemExit) as ex:
        cli.check_args(p, p.parse_args(BASE + extra))
    assert ex.value.code == 2 and "error:" in capsys.readouterr().err


def test_synth_cli_json_line_overrides_the_flags(tmp_path):
    from kokoro.cli import synth as cli
    f = tmp_path / "u.jsonl"
    f.write_text('{"name": "a", "phoneme_indices": [1, 2, 3]}\n\n'
                 '{"name": "b", "phoneme_indices": [4, 5], "prosody": {"speed": 2.0, "durations": [3, -1], "pitch": [null, 0.5]}}\n')
    assert cli.read_prosody(str(f), {}) is not None
    got = cli.read_prosody(str(f), {"speed": 0.5, "energy_scale": 1.5})
    assert len(got) == 2
    assert got[0].speed == 0.5 and got[0].energy_scale == 1.5 and got[0].durations is None
    assert got[1].speed == 2.0 and got[1].energy_scale == 1.5 and got[1].durations == [3, -1] and math.isnan(got[1].pitch[0])
    names, ids, st = cli.read_ids(str(f))
    assert names == ["a", "b"] and st is None
    f.write_text('{"name": "a", "phoneme_indices": [1, 2, 3]}\n')
    assert cli.read_prosody(str(f), {}) is None, "nothing asked for: the engine is called without controls"
    f.write_text('{"name": "a", "phoneme_indices": [1, 2, 3], "prosody": {"durations": [1, 2]}}\n')
    with pytest.raises(ValueError, match="u.jsonl:1"):
        cli.read_prosody(str(f), {})


class _Engine:
    device = "cpu"

    class dims:
        mel = 4

    def __init__(self):
        self.calls = []

    def generate_batch(self, utterances, stress=None, *, want_info=False, **kw):
        self.calls.append(("batch", [int(u.numel()) for u in utterances], kw))
        mels = [torch.zeros(int(u.numel()), 4) for u in utterances]
        info = {"durations": [torch.ones(int(u.numel())) for u in utterances], "T": [int(u.numel()) for u in utterances],
                "bounds": [(1, int(u.numel()), 50) for u in utterances]}
        return (mels, info) if want_info else mels

    def generate_stream(self, utterances, stress=None, *, slots=32, want_info=False, **kw):
        self.calls.append(("stream", [int(u.numel()) for u in utterances], kw))
        return self.generate_batch(utterances, stress, want_info=want_info)


def test_synthesize_hands_each_batch_its_utterances_controls():
    from kokoro.inference.synth import synthesize
    e = _Engine()
    utts = [torch.ones(n, dtype=torch.int64) for n in (5, 2, 9)]
    pr = [Prosody(speed=1.0 + i) for i in range(3)]
    synthesize(e, utts, None, batch_size=2, prosody=pr, max_len=7)
    assert [(c[0], c[1]) for c in e.calls] == [("batch", [2, 5]), ("batch", [9])]
    assert e.calls[0][2] == {"max_len": 7, "prosody": [pr[1], pr[0]]} and e.calls[1][2] == {"max_len": 7, "prosody": [pr[2]]}
    e.calls.clear()
    synthesize(e, utts, None, stream=True, prosody=pr[0], max_len=7)
    assert e.calls[0][0] == "stream" and e.calls[0][2] == {"max_len": 7, "prosody": [pr[0]] * 3}
    e.calls.clear()
    synthesize(e, utts, None, batch_size=4, max_len=7)
    assert e.calls[0][2] == {"max_len": 7}, "without controls the engine is called as before"
    with pytest.raises(ValueError):
        synthesize(e, utts, None, prosody=pr[:2])


def test_evaluate_passes_prosody_and_eval_cli_oracle_durations():
    from kokoro.cli import evaluate as ecli
    from kokoro.inference import evaluate as E

    class Al:
        def align(self, syn, ref, **kw):
            return [{"mcd_dtw": 0.0, "mel_l1_dtw": 0.0, "len_ratio": 1.0} for _ in syn]

    e = _Engine()
    utts = [torch.ones(n, dtype=torch.int64) for n in (3, 2)]
    refs = [torch.zeros(4, 4), torch.zeros(4, 4)]
    pr = [Prosody(durations=[1, 1, 1]), Prosody(durations=[2, 2])]
    E.evaluate(e, utts, None, refs, stream=True, aligner=Al(), prosody=pr)
    assert e.calls[0][2] == {"prosody": pr}
    e.calls.clear()
    E.evaluate(e, utts, None, refs, stream=False, batch_size=1, aligner=Al(), prosody=pr)
    assert [c[2] for c in e.calls if c[0] == "batch"] == [{"prosody": [pr[1]]}, {"prosody": [pr[0]]}]
    p = ecli.build_parser()
    assert p.parse_args(["--checkpoint", "c", "--features", "d"]).oracle_durations is False
    assert p.parse_args(["--checkpoint", "c", "--features", "d", "--oracle-durations"]).oracle_durations is True
    got = ecli.oracle_prosody(["a", "b"], utts, [torch.tensor([4, 0, 2]), torch.tensor([1, 1])])
    assert [g.durations.tolist() for g in got] == [[4, 0, 2], [1, 1]]
    with pytest.raises(ValueError, match="utterance b"):
        ecli.oracle_prosody(["a", "b"], utts, [torch.tensor([4, 0, 2]), torch.tensor([1])])
