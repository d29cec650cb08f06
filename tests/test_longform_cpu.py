"""Long-form synthesis without a GPU: the fp64 oracle (kokoro_ruslan_amd/longform_torch.py) against the host function it restates and
against torch.cat, and the --documents side of the kokoro-synth command line."""
import json
import os
import sys

import pytest
import torch

from kokoro.cli import synth as cli
from kokoro.inference.synth import trim_trailing_silence
from kokoro_ruslan_amd.longform_torch import fade_table, finish_reference, join_reference

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_cases as LC  # noqa: E402

CASES = LC.finish_cases()
MARGIN = 1e-3        # what a decision must keep clear of: an fp32 frame mean of 80 values of magnitude <= 11.5 is off by <= 5.4e-5


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def test_case_table_covers_every_branch():
    assert {int(m.shape[0]) for _, m, _ in CASES} >= set(LC.T_REQUIRED)
    assert all(m.shape[1] == 80 and m.dtype == torch.float32 for _, m, _ in CASES)
    seen = {}
    for name, mel, branch in CASES:
        _, t_end, last, thr, st = finish_reference(mel)
        T = mel.shape[0]
        assert st["frame_margin"] >= MARGIN and st["branch_margin"] >= MARGIN, (name, st)
        kind = "nan" if st["nan"] else ("under" if thr == -9.8 else "over" if thr == -9.2 else "inside")
        assert kind == branch and (kind != "inside" or -9.8 < thr < -9.2), (name, thr)
        seen.setdefault("branch", set()).add(kind)
        if last < 0:
            seen["unvoiced"] = True
            assert t_end == T
        else:
            seen["near" if last + 24 + 1 >= T else "far"] = True
            if last + 24 + 1 < 60 <= T:
                seen["min_keep"] = True
                assert t_end == 60
        if float(mel[~torch.isnan(mel)].min()) < -11.5 and float(mel[~torch.isnan(mel)].max()) > 2.0:
            seen["outside"] = True
    assert seen["branch"] == {"under", "over", "inside", "nan"}
    assert all(seen.get(k) for k in ("unvoiced", "near", "far", "min_keep", "outside")), seen


@pytest.mark.parametrize("name,mel,branch", CASES, ids=[c[0] for c in CASES])
def test_oracle_agrees_with_the_host_function(name, mel, branch):
    clamped, t_end, last, thr, st = finish_reference(mel)
    assert st["frame_margin"] >= MARGIN and st["branch_margin"] >= MARGIN        # the decisions are the same in fp32
    host = trim_trailing_silence(mel)
    assert host.shape[0] == t_end, (name, host.shape[0], t_end, last, thr)
    assert clamped.dtype == torch.float32 and torch.equal(_bits(host), _bits(clamped[:t_end]))
    assert torch.equal(_bits(clamped), _bits(torch.clamp(mel, min=-11.5, max=2.0)))


def test_oracle_statistics():
    g = torch.Generator().manual_seed(3)
    mel = torch.randn(37, 80, generator=g) * 2.0 - 5.0
    _, _, _, _, st = finish_reference(mel)
    x = mel.double()
    assert st["min"] == float(x.min()) and st["max"] == float(x.max()) and st["nan"] == 0
    assert abs(st["mean"] - float(x.mean())) <= 1e-12 and abs(st["std"] - float(x.std())) <= 1e-12
    flat = torch.full((70, 80), -3.3)
    assert finish_reference(flat)[4]["std"] < 1e-5
    mel[5, 5] = float("nan")
    _, t_end, _, thr, st = finish_reference(mel)
    assert st["nan"] == 1 and thr == -9.2 and st["std"] != st["std"] and st["min"] == float(x[x == x].min())
    assert t_end == trim_trailing_silence(mel).shape[0]
    with pytest.raises(ValueError, match="frames >= 1"):
        finish_reference(torch.zeros(0, 80))


@pytest.mark.parametrize("gap", LC.GAPS)
def test_join_oracle_is_torch_cat(gap):
    chunks = LC.join_chunks_input()
    waves, peaks = join_reference(chunks, LC.DOCUMENTS, gap, 0)
    want = LC.cat_documents(chunks, LC.DOCUMENTS, gap)
    assert len(waves) == len(want) == 4
    for w, e in zip(waves, want):
        assert torch.equal(_bits(w), _bits(e))
    assert torch.equal(peaks, torch.stack([c.abs().max() for c in chunks]))
    one = [[i] for i in range(len(chunks))]
    for w, c in zip(join_reference(chunks, one, gap, 0)[0], chunks):
        assert torch.equal(w, c)                                           # no gap at a document's ends


def test_join_oracle_fades_half_a_short_chunk():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(100, generator=g) + 0.5
    (w,), peaks = join_reference([x], [[0]], 0, 64)
    t = fade_table(64)
    assert t.dtype == torch.float32 and 0 < float(t[0]) < float(t[63]) < 1 and abs(float(t[0]) + float(t[63]) - 1) < 1e-6
    assert torch.equal(w[:50], x[:50] * t[:50]) and torch.equal(w[50:], x[50:] * t[:50].flip(0))
    assert float(peaks[0]) == float(x.abs().max())
    y = torch.rand(1000, generator=g)
    (w,), _ = join_reference([y], [[0]], 0, 64)
    assert torch.equal(w[64:936], y[64:936]) and torch.equal(w[:64], y[:64] * t) and torch.equal(w[936:], y[936:] * t.flip(0))


def test_join_oracle_refuses_bad_documents():
    chunks = LC.join_chunks_input()[:3]
    for docs in ([[0, 1]], [[0, 1, 1, 2]], [[0, 1], [], [2]], [[0, 1, 3]]):
        with pytest.raises(ValueError, match="documents"):
            join_reference(chunks, docs, 10)


SYNTH = ["--checkpoint", "ck", "--ids", "u.jsonl", "--output", "out"]


def _refused(argv, capsys, match):
    p = cli.build_parser()
    with pytest.raises(SystemExit) as e:
        cli.check_args(p, p.parse_args(argv))
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def test_cli_argument_checks(capsys):
    _refused(SYNTH + ["--gap-ms", "100"], capsys, "--gap-ms / --fade-ms need --documents")
    _refused(SYNTH + ["--griffin-lim", "--fade-ms", "5"], capsys, "--gap-ms / --fade-ms need --documents")
    _refused(SYNTH + ["--documents"], capsys, "--documents needs --vocoder or --griffin-lim")
    _refused(["--checkpoint", "ck", "--features", "c", "--output", "o", "--griffin-lim", "--documents"], capsys, "--documents needs --ids")
    _refused(SYNTH + ["--griffin-lim", "--documents", "--fade-ms", "-1"], capsys, "--fade-ms must be >= 0")
    _refused(SYNTH + ["--griffin-lim", "--documents", "--gap-ms", "-0.5"], capsys, "--gap-ms must be >= 0")
    p = cli.build_parser()
    a = p.parse_args(SYNTH + ["--griffin-lim", "--documents", "--report", "r.json"])
    cli.check_args(p, a)
    assert cli.long_form(a) == (True, 150.0, 0.0, "r.json")
    a = p.parse_args(SYNTH + ["--vocoder", "v", "--documents", "--gap-ms", "0", "--fade-ms", "2.5"])
    cli.check_args(p, a)
    assert cli.long_form(a) == (True, 0.0, 2.5, None)
    assert cli.long_form(p.parse_args(SYNTH)) == (False, 150.0, 0.0, None)


def _write(path, records):
    path.write_text("".join(json.dumps(r) + "\n" for r in records))
    return str(path)


def test_read_documents(tmp_path):
    rec = lambda name, **kw: dict({"name": name, "phoneme_indices": [1, 2]}, **kw)
    f = _write(tmp_path / "a.jsonl", [rec("s0", document="story"), rec("alone"), rec("t0", document="talk"), rec("s1", document="story"),
                                      rec("s2", document="story")])
    assert cli.read_documents(f) == (["story", "alone", "talk"], [[0, 3, 4], [1], [2]])
    assert cli.read_ids(f)[0] == ["s0", "alone", "t0", "s1", "s2"] and len(cli.read_ids(f)) == 3
    f = _write(tmp_path / "b.jsonl", [rec("story", document="story"), rec("s1", document="story")])
    assert cli.read_documents(f) == (["story"], [[0, 1]])                  # a chunk may carry its own document's name
    f = _write(tmp_path / "c.jsonl", [rec("story"), rec("s1", document="story")])
    with pytest.raises(ValueError, match="'story'"):
        cli.read_documents(f)
    f = _write(tmp_path / "d.jsonl", [rec("talk", document="story"), rec("t0", document="talk")])
    with pytest.raises(ValueError, match="'talk' names a document and a chunk"):
        cli.read_documents(f)
    f = _write(tmp_path / "e.jsonl", [rec("x", document="")])
    with pytest.raises(ValueError, match="non-empty string"):
        cli.read_documents(f)
