"""CPU suite: `kokoro-synth --stream [--slots N]` and `synthesize(..., stream=True, slots=N)` hand the utterances to
KokoroEngine.generate_stream; the default paths stay on generate_batch.  The engine is a stub."""
import json

import numpy as np
import pytest
import torch

from kokoro.cli import synth as cli
from kokoro.inference import synth as S


class StubEngine:
    device = "cpu"

    class dims:
        mel = 4

    def __init__(self):
        self.calls = []

    def _mels(self, utterances):
        return [torch.full((int(u.numel()) + 1, 4), float(u.sum())) for u in utterances]

    def generate_batch(self, utterances, stress=None, **kw):
        self.calls.append(("batch", len(utterances), stress is not None, kw))
        return self._mels(utterances)

    def generate_stream(self, utterances, stress=None, *, slots=32, **kw):
        self.calls.append(("stream", len(utterances), stress is not None, slots, kw))
        return self._mels(utterances)


UTTS = [torch.tensor([3, 4, 5]), torch.tensor([7]), torch.tensor([1, 2])]


def test_synthesize_stream_is_one_generate_stream_call_in_input_order():
    e = StubEngine()
    mels = S.synthesize(e, UTTS, None, stream=True, slots=5, max_len=40)
    assert e.calls == [("stream", 3, False, 5, {"max_len": 40})]
    assert [m.shape[0] for m in mels] == [4, 2, 3] and [float(m[0, 0]) for m in mels] == [12.0, 7.0, 3.0]
    st = [torch.zeros_like(u) for u in UTTS]
    S.synthesize(e, UTTS, st, stream=True)
    assert e.calls[-1] == ("stream", 3, True, 32, {})
    with pytest.raises(ValueError):
        S.synthesize(e, UTTS, None, stream=True, slots=0)
    with pytest.raises(ValueError):
        S.synthesize(e, UTTS, st[:2], stream=True)


def test_synthesize_default_stays_on_generate_batch():
    e = StubEngine()
    mels = S.synthesize(e, UTTS, None, batch_size=2, max_len=40)
    assert [c[0] for c in e.calls] == ["batch", "batch"] and all(c[3] == {"max_len": 40} for c in e.calls)
    assert [float(m[0, 0]) for m in mels] == [12.0, 7.0, 3.0]


def test_parser_stream_flags():
    base = ["--checkpoint", "c", "--ids", "x.jsonl", "--output", "o"]
    a = cli.build_parser().parse_args(base)
    assert a.stream is False and a.slots is None
    a = cli.build_parser().parse_args(base + ["--stream"])
    assert a.stream is True and a.slots is None
    a = cli.build_parser().parse_args(base + ["--stream", "--slots", "8"])
    assert a.stream is True and a.slots == 8
    p = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_args(p, p.parse_args(base + ["--slots", "8"]))
    with pytest.raises(SystemExit):
        cli.check_args(p, p.parse_args(base + ["--stream", "--slots", "0"]))


@pytest.mark.parametrize("extra,want", [([], ("batch", None)), (["--stream"], ("stream", 32)), (["--stream", "--slots", "4"], ("stream", 4))])
def test_kokoro_synth_hands_stream_and_slots_to_synthesize(tmp_path, monkeypatch, extra, want):
    e = StubEngine()
    seen = {}
    monkeypatch.setattr(S, "load_for_inference", lambda path, **kw: (e, S.InferenceControls(max_len=40), "model"))
    real = S.synthesize

    def spy(engine, utterances, stress=None, **kw):
        seen.update(kw)
        return real(engine, utterances, stress, **kw)
    monkeypatch.setattr(S, "synthesize", spy)
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps({"name": f"u{i}", "phoneme_indices": u.tolist()}) + "\n" for i, u in enumerate(UTTS)))
    out = tmp_path / "mels"
    assert cli.main(["--checkpoint", "ck", "--ids", str(ids_file), "--output", str(out), "--batch-size", "2"] + extra) == 0
    kind, slots = want
    assert {c[0] for c in e.calls} == {kind}
    if kind == "stream":
        assert seen["stream"] is True and seen["slots"] == slots and e.calls[0][3] == slots and "batch_size" not in seen
    else:
        assert not seen.get("stream", False) and seen["batch_size"] == 2
    assert seen["max_len"] == 40
    for i, u in enumerate(UTTS):
        a = np.load(out / f"u{i}.npy")
        assert a.shape == (4, int(u.numel()) + 1) and float(a[0, 0]) == float(u.sum())
