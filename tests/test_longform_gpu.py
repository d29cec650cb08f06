"""`kokoro-synth --documents` end to end on the device: a tiny engine with random weights, Griffin-Lim with seeded phases, an ids file
of two documents (three chunks and one) and a line of its own.  Every <document>.wav equals, byte for byte, what the public calls that
existed before give: synthesize -> trim_trailing_silence on the host -> vocode -> torch.cat with 0.15 s of zeros -> write_wav."""
import json
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd.longform_torch import finish_reference

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def test_kokoro_synth_documents(tmp_path):
    _need_gpu()
    from kokoro.cli import synth as cli
    from kokoro.inference import vocode
    from kokoro.inference.audio import write_wav
    from kokoro.inference.synth import load_for_inference, synthesize, trim_trailing_silence
    from kokoro.training.checkpoint import save_checkpoint
    from kokoro.training.config import TrainingConfig
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d = ModelDims(vocab=59, mel=80, hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32, var_kernel=3,
                  var_bins=16, max_len=300)
    e = KokoroEngine(d, StepHyper(), math_mode="f32", total_steps=100, seed=5)
    cfg = TrainingConfig(n_mels=80, hidden_dim=128, n_encoder_layers=1, n_decoder_layers=1, n_heads=2, encoder_ff_dim=96,
                         decoder_ff_dim=96, max_decoder_seq_len=300, variance_filter_size=32, n_variance_bins=16)
    ck = save_checkpoint(e, cfg, 0, 1.0, str(tmp_path / "ck"))
    g = torch.Generator().manual_seed(2)
    lines = [("s0", "story", 5), ("alone", None, 17), ("t0", "talk", 9), ("s1", "story", 12), ("s2", "story", 7)]
    ids = [torch.randint(1, 59, (n,), generator=g) for _, _, n in lines]
    ids_file = tmp_path / "u.jsonl"
    ids_file.write_text("".join(json.dumps(dict({"name": name, "phoneme_indices": v.tolist()}, **({"document": doc} if doc else {}))) + "\n"
                                for (name, doc, _), v in zip(lines, ids)))
    out, report = tmp_path / "out", tmp_path / "report.json"
    assert cli.main(["--checkpoint", str(ck), "--ids", str(ids_file), "--batch-size", "2", "--math", "f32", "--max-len", "40",
                     "--min-len-floor", "8", "--weights", "model", "--output", str(out), "--documents", "--griffin-lim",
                     "--griffin-lim-iters", "5", "--griffin-lim-seed", "7", "--report", str(report)]) == 0
    names = [n for n, _, _ in lines]
    assert sorted(os.listdir(out)) == sorted([f"{n}.npy" for n in names] + ["story.wav", "talk.wav", "alone.wav"])

    engine, controls, _ = load_for_inference(str(ck), weights="model", math_mode="f32", max_len=40, min_len_floor=8)
    mels = [m.float().cpu() for m in synthesize(engine, ids, None, batch_size=2, **controls.kwargs())]
    for name, m in zip(names, mels):                                       # the host's fp32 decisions are the oracle's, so the device's
        st = finish_reference(m)[4]
        assert st["frame_margin"] >= 1e-3 and st["branch_margin"] >= 1e-3, (name, st)
    host = [trim_trailing_silence(m) for m in mels]
    for name, m in zip(names, host):
        assert np.array_equal(np.load(out / f"{name}.npy"), m.t().numpy()), name
    audio = vocode(GriffinLimVocoder(), host, n_iter=5, generator=torch.Generator().manual_seed(7))
    silence = torch.zeros(3307, device=audio[0].device)
    for doc, members in (("story", [0, 3, 4]), ("alone", [1]), ("talk", [2])):
        parts = []
        for k, c in enumerate(members):
            parts += ([silence] if k else []) + [audio[c]]
        write_wav(str(tmp_path / "want.wav"), torch.cat(parts), 22050)
        assert (out / f"{doc}.wav").read_bytes() == (tmp_path / "want.wav").read_bytes(), doc

    entries = json.loads(report.read_text())
    assert [r["name"] for r in entries] == names
    assert [r["document"] for r in entries] == ["story", "alone", "talk", "story", "story"]
    for r, m, a in zip(entries, host, audio):
        assert r["kept"] == m.shape[0] == np.load(out / f"{r['name']}.npy").shape[1] and r["nan"] == 0 and r["flat"] is False
        assert r["audio_peak"] == float(a.abs().max()) and r["silent"] == (r["audio_peak"] < 1e-4)
        assert set(r) == {"name", "document", "frames", "kept", "last_voiced", "threshold", "min", "max", "mean", "std", "nan", "flat",
                          "audio_peak", "silent"}
