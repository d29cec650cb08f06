"""GPU suite: PhoneAligner(mixtures=2 | 4) end to end: mixtures = 1 is the aligner it always was, the mixture training on
align_torch.synthetic_corpus_modes against the fp64 oracle's gain, every mixture pass's scores against its own durations, batch
independence, the model file through kokoro-align --mixtures and kokoro-eval's --pronunciation, and the unchanged default output.

The score of an utterance is held against align_torch.path_score_states of its own state durations under the kernel's own L by the
bound of tests/test_align_kernels_gpu.py: the kernel's sequential fp32 sum along its path differs from that path's exact sum by at most
T 2^-23 sum_t max_c |L(c, t)|."""
import argparse
import json
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
V, D = 12, 8
ITERS = 12


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.align import PhoneAligner
    return PhoneAligner


@pytest.fixture(scope="module")
def corpus():
    """synthetic_corpus_modes(0) and what the fp64 oracle makes of it with one Gaussian and with two; computed once, never changed."""
    feats, ids, _, truth, _, _ = R.synthetic_corpus_modes(0)
    _, d1, _ = R.fit(feats, ids, V=V, iters=ITERS)
    _, sd2, _ = R.fit_mix(feats, ids, V=V, S=1, M=2, iters=ITERS)
    acc1, acc2 = R.frame_accuracy(ids, d1, truth), R.frame_accuracy(ids, [d.sum(1) for d in sd2], truth)
    return dict(feats=feats, ids=ids, truth=truth, tfeats=[torch.from_numpy(x) for x in feats], tids=[torch.from_numpy(i) for i in ids],
                oracle=(acc1, acc2))


def test_mixtures_1_is_the_aligner_it_always_was(gpu, corpus):
    from kokoro_ruslan_amd import lib as kk
    for S in (1, 2):
        a, b = gpu(n_classes=V, **({"states": S} if S > 1 else {})), gpu(n_classes=V, states=S, mixtures=1)
        n0 = kk.launches
        m0, d0, s0 = a.fit(None, corpus["tids"], iters=4, batch_size=16, feats=corpus["tfeats"])
        n1 = kk.launches
        m1, d1, s1 = b.fit(None, corpus["tids"], iters=4, batch_size=16, feats=corpus["tfeats"])
        assert kk.launches - n1 == n1 - n0, "the same launches"
        assert s0 == s1 and set(m0) == set(m1) and "mixtures" not in m1 and "weight" not in m1
        assert torch.equal(m0["mean"], m1["mean"]) and torch.equal(m0["var"], m1["var"])
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(d0, d1))
        if S > 1:
            assert all(torch.equal(x, y) for x, y in zip(a.state_durations, b.state_durations))


def _fit_and_check_passes(gpu, corpus, S, M, mix_iters=4):
    """fit at (S, M) on the corpus; every mixture alignment's scores against the fp64 score of its own durations under its own L."""
    al = gpu(n_classes=V, states=S, mixtures=M)
    seen = []

    def check(model, runs):
        n, worst = 0, 0.0
        for run in runs:
            L = run["L"].cpu().numpy().astype(np.float64)
            score = run["score"].cpu().numpy().astype(np.float64)
            sd = (run["state_durations"] if S > 1 else run["durations"][:, None]).cpu().numpy().astype(np.int64)
            assert L.shape[0] == V * S
            for u in range(len(score)):
                f0, f1, p0, p1 = run["foff_host"][u], run["foff_host"][u + 1], run["poff_host"][u], run["poff_host"][u + 1]
                if not math.isfinite(score[u]):
                    assert score[u] == -math.inf and not sd[p0:p1].any(), "an infeasible utterance has no durations"
                    continue
                assert int(sd[p0:p1].sum()) == f1 - f0
                want = R.path_score_states(L[:, f0:f1], corpus["ids"][n + u], sd[p0:p1], S)
                bound = (f1 - f0) * EPS * float(np.abs(L[:, f0:f1]).max(0).sum())
                worst = max(worst, abs(score[u] - want) / bound)
                assert abs(score[u] - want) <= bound, (len(seen), n + u, score[u], want, bound)
            n += len(score)
        assert n == len(corpus["ids"])
        seen.append((int(model["mixtures"]), worst))
    model, durs, scores = al.fit(None, corpus["tids"], iters=ITERS, batch_size=16, feats=corpus["tfeats"], mix_iters=mix_iters, on_mix_pass=check)
    print(f"S {S} M {M}: {len(scores)} passes, the mixture alignments (components, largest |score - fp64 of its durations| / bound): {seen}")
    doublings = int(math.log2(M))
    assert doublings + 1 <= len(seen) <= doublings * mix_iters + 1 and seen[0][0] == 2 and seen[-1][0] == M
    assert [m for m, _ in seen] == sorted(m for m, _ in seen)
    assert model["mixtures"] == M and model["mean"].shape == model["var"].shape == (V * S * M, D) and model["weight"].shape == (V * S, M)
    assert model["mean"].dtype == model["weight"].dtype == torch.float64 and (model["weight"] > 0).all()
    assert float((model["weight"].sum(1) - 1.0).abs().max()) <= 1e-12
    assert ("states" in model) == (S > 1)
    # the durations returned are the model's own
    recs = al.align(None, corpus["tids"], (), model, feats=corpus["tfeats"])
    assert all((d is None and r["durations"] is None) or torch.equal(d, r["durations"]) for d, r in zip(durs, recs))
    if S > 1:
        assert all((x is None and r["state_durations"] is None) or torch.equal(x, r["state_durations"]) for x, r in zip(al.state_durations, recs))
    else:
        assert al.state_durations is None
    return al, model, durs, scores


def test_two_components_gain_at_least_half_of_what_the_oracle_gains(gpu, corpus):
    one = gpu(n_classes=V)
    _, d1, s1 = one.fit(None, corpus["tids"], iters=ITERS, batch_size=16, feats=corpus["tfeats"])
    _, _, d2, s2 = _fit_and_check_passes(gpu, corpus, 1, 2)
    acc1 = R.frame_accuracy(corpus["ids"], [d.numpy() for d in d1], corpus["truth"])
    acc2 = R.frame_accuracy(corpus["ids"], [d.numpy() for d in d2], corpus["truth"])
    o1, o2 = corpus["oracle"]
    print(f"frame accuracy: device {acc1:.4f} -> {acc2:.4f}, fp64 oracle {o1:.4f} -> {o2:.4f}")
    assert o2 - o1 >= 0.02, "the corpus shows a gain worth testing"
    assert acc2 - acc1 >= 0.5 * (o2 - o1)
    assert s2[:len(s1)] == s1, "the single-Gaussian training runs first, all of it"
    assert all(d.dtype == torch.int64 and int(d.sum()) == x.shape[0] for d, x in zip(d2, corpus["feats"]))


@pytest.mark.parametrize("S,M", [(2, 2), (1, 4)])
def test_every_mixture_pass_scores_its_own_durations(gpu, corpus, S, M):
    _fit_and_check_passes(gpu, corpus, S, M, mix_iters=2)


def test_an_utterances_result_with_a_mixture_model_does_not_depend_on_the_batch(gpu, corpus):
    S, M = 2, 4
    g = torch.Generator().manual_seed(3)
    al = gpu(n_classes=V, states=S, mixtures=M)
    w = torch.rand(V * S, M, generator=g, dtype=torch.float64) + 0.1
    model = {"mean": torch.randn(V * S * M, D, generator=g, dtype=torch.float64) * 2.0, "var": torch.rand(V * S * M, D, generator=g, dtype=torch.float64) + 0.5,
             "weight": w / w.sum(1, keepdim=True), "states": S, "mixtures": M}
    pick = [0, 5, 11, 17]
    feats, ids = [corpus["tfeats"][n] for n in pick], [corpus["tids"][n] for n in pick]
    feats.append(torch.randn(9, D, generator=g)), ids.append(torch.randint(0, V, (5,), generator=g))      # 5 tokens of 2 states on 9 frames
    batch, scored = al.align(None, ids, (), model, feats=feats), al.score(None, ids, (), model, feats=feats)
    assert [r["feasible"] for r in batch] == [True] * 4 + [False]
    for n in range(len(ids)):
        alone = al.align(None, [ids[n]], (), model, feats=[feats[n]])[0]
        sc = al.score(None, [ids[n]], (), model, feats=[feats[n]])[0]
        assert alone["score"] == batch[n]["score"] == scored[n]["score"] == sc["score"]
        if not alone["feasible"]:
            assert batch[n]["durations"] is None and sc["gop"] is None and scored[n]["gop"] is None
            continue
        assert torch.equal(alone["durations"], batch[n]["durations"]) and torch.equal(alone["state_durations"], batch[n]["state_durations"])
        for k in ("gop", "logpost", "phone_acc", "gop_min", "gop_min_token"):
            assert sc[k] == scored[n][k], k
        for k in ("frames", "hits", "gop", "logpost"):
            assert torch.equal(sc["tokens"][k].view(torch.int64), scored[n]["tokens"][k].view(torch.int64)), k


def _entry(g, name, T, P, templates):
    from kokoro.data import features as DF
    ids = torch.randint(1, 59, (P,), generator=g)
    mode = torch.randint(0, 2, (P,), generator=g)
    d = torch.from_numpy(R.even_split(P, T))
    mel = templates[torch.repeat_interleave(ids * 2 + mode, d)] + 0.3 * torch.randn(T, 80, generator=g)
    ft = {"mel_spec": mel.t().contiguous(), "pitch": torch.rand(T, generator=g), "energy": torch.rand(T, generator=g), "mel_length": T}
    return DF.cache_entry(ft, name, ids, None, None, "text " + name)


def test_kokoro_align_mixtures_and_the_tools_that_take_its_model(gpu, tmp_path, capsys):
    from kokoro.cli import align as cli
    from kokoro.cli import evaluate as ev
    from kokoro.data import features as DF
    from kokoro.inference.evaluate import _pron_records
    g = torch.Generator().manual_seed(4)
    templates = torch.randn(59 * 2, 80, generator=g)
    cache = tmp_path / "cache"
    shapes = {"u0": (12, 3), "u1": (30, 7), "u2": (42, 21), "u3": (17, 1), "u4": (40, 16), "u5": (25, 6)}
    for name, (T, P) in shapes.items():
        DF.write_cache_entry(str(cache), _entry(g, name, T, P, templates))
    base = ["--cache-dir", str(cache), "--iters", "3", "--batch-size", "4"]
    # without the flag: what it always was, and --mixtures 1 is the same run
    out0, out1, m0, m1 = tmp_path / "d0.jsonl", tmp_path / "d1.jsonl", tmp_path / "m0.pt", tmp_path / "m1.pt"
    assert cli.main(base + ["--output", str(out0), "--model-out", str(m0)]) == 0
    text0 = capsys.readouterr().out
    assert cli.main(base + ["--output", str(out1), "--model-out", str(m1), "--mixtures", "1"]) == 0
    assert capsys.readouterr().out == text0 and out0.read_bytes() == out1.read_bytes()
    f0, f1 = torch.load(m0, weights_only=True), torch.load(m1, weights_only=True)
    assert set(f0) == set(f1) == {"mean", "var", "K", "n_classes"} and all(torch.equal(torch.as_tensor(f0[k]), torch.as_tensor(f1[k])) for k in f0)
    entries = cli.read_cache(str(cache))
    _, durs, _ = gpu().fit([e["mel"] for e in entries], [e["ids"] for e in entries], iters=3, batch_size=4)
    want = "".join(json.dumps({"name": e["name"], "phoneme_durations": [int(v) for v in d]}) + "\n" for e, d in zip(entries, durs))
    assert out0.read_text() == want and set(torch.load(m0, weights_only=True)) == {"mean", "var", "K", "n_classes"}
    # --mixtures 2
    out2, m2 = tmp_path / "d2.jsonl", tmp_path / "m2.pt"
    assert cli.main(base + ["--output", str(out2), "--model-out", str(m2), "--mixtures", "2", "--mix-iters", "2"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith("kokoro-align: 6 aligned, 0 infeasible (6 utterances), ")
    lines = [json.loads(l) for l in open(out2)]
    assert all(set(l) == {"name", "phoneme_durations"} and sum(l["phoneme_durations"]) == shapes[l["name"]][0] for l in lines)
    saved = torch.load(m2, weights_only=True)
    assert saved["mixtures"] == 2 and saved["mean"].shape == (118, 28) and saved["weight"].shape == (59, 2) and gpu.file_mixtures(str(m2)) == 2
    # the file's mixtures hold with --model-in and the durations come back; a conflicting --mixtures names both
    out3 = tmp_path / "d3.jsonl"
    assert cli.main(["--cache-dir", str(cache), "--batch-size", "4", "--model-in", str(m2), "--output", str(out3)]) == 0
    assert out3.read_bytes() == out2.read_bytes()
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--output", str(out3), "--mixtures", "2", "--scores"]) == 0
    assert [json.loads(l)["phoneme_durations"] for l in open(out3)] == [l["phoneme_durations"] for l in lines]
    capsys.readouterr()
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--mixtures", "4"]) == 1
    err = capsys.readouterr().err
    assert "--mixtures 4" in err and "mixtures = 2" in err
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m0), "--mixtures", "2"]) == 1
    err = capsys.readouterr().err
    assert "--mixtures 2" in err and "mixtures = 1" in err
    # kokoro-eval --pronunciation FILE: the file's mixtures hold, and evaluate() builds the aligner the model asks for
    mels, ids = [e["mel"] for e in entries], [e["ids"] for e in entries]
    kw, how = ev.phone_scoring(argparse.Namespace(pronunciation=str(m2)), "cuda", 59, mels, ids)
    assert how == f"model {m2}" and kw["phone_model"]["mixtures"] == 2 and kw["phone_aligner"].aligner.mixtures == 2
    direct = kw["phone_aligner"].score(mels, ids, (), kw["phone_model"])
    assert [e["name"] for e in entries] == [l["name"] for l in lines]
    assert [r["durations"].tolist() for r in direct] == [l["phoneme_durations"] for l in lines]
    recs = _pron_records(None, kw["phone_model"], (), "cuda", mels, mels, ids)
    assert [r["gop"] for r in recs] == [r["gop"] for r in direct] and all(r["gop_gap"] == 0.0 for r in recs)
    kw4, how4 = ev.phone_scoring(argparse.Namespace(pronunciation="", align_mixtures=4, align_iters=2), "cuda", 59, mels, ids)
    assert kw4["phone_model"]["mixtures"] == 4 and "fitted on the selection" in how4
