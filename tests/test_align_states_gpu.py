"""GPU suite: PhoneAligner(states=2 | 3) against the fp64 oracle's fit_states on a synthetic corpus of phones that are not stationary,
the pronunciation scores of a 2-state model, the model file's `states`, and kokoro-align --states on a temporary feature cache.

The corpus is align_torch.synthetic_corpus_parts(0, parts=S), passed as features.  Per pass the device's corpus score must lie within
the summed kernel bound of the oracle's, exactly as tests/test_align_gpu.py derives it: per utterance T 2^-23 A for the recurrence
plus, per frame, (D + 8) 2^-23 E(c, t) for the fp32 log-likelihood, now over the V S classes.  The scores are held against
align_torch.scores on phone_max of the kernel's OWN L, labels // S and phone durations, by the rules of
tests/test_align_scores_kernels_gpu.py (amax, hits, margins and gop sums exact, the log posteriors within that file's bound)."""
import json
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
U = 2.0 ** -53
V, D = 12, 8
ITERS = 12                                                # the oracle converges in 3, 4, 5 and 8 passes on the four corpora below


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.align import PhoneAligner
    return PhoneAligner


def _pass_bound(feats, model):
    a, mu, c = R.loglik_params(model)
    total = 0.0
    for x in feats:
        x = np.asarray(x, dtype=np.float64)
        A = float(np.abs(R.loglik_from_params(x, a, mu, c)).max(0).sum())
        E = np.stack([(np.abs(a[v]) * (np.abs(x) + np.abs(mu[v])) ** 2).sum(1) + abs(c[v]) for v in range(a.shape[0])])
        total += x.shape[0] * EPS * A + (D + 8) * EPS * float(E.max(0).sum())
    return total


@pytest.mark.parametrize("S,optional,cap", [(2, False, 0.99), (2, True, 0.97), (3, False, 0.99), (3, True, 0.97)])
def test_fit_follows_the_oracle_pass_by_pass(gpu, S, optional, cap):
    feats, ids, opts, truth, _, _ = R.synthetic_corpus_parts(0, S, optional)
    models = []
    _, want, ref_scores = R.fit_states(feats, ids, opts if optional else None, V=V, S=S, iters=ITERS, models=models)
    al = gpu(n_classes=V, states=S)
    model, durs, scores = al.fit(None, [torch.from_numpy(i) for i in ids], (0,) if optional else (), iters=ITERS, batch_size=16,
                                 feats=[torch.from_numpy(x) for x in feats])
    assert len(scores) == len(ref_scores) < ITERS, (scores, ref_scores)
    for n, (s, r, m) in enumerate(zip(scores, ref_scores, models)):
        bound = _pass_bound(feats, m)
        print(f"S {S} optional {optional} pass {n}: device {s!r}  oracle {r!r}  |difference| {abs(s - r):.3e}  bound {bound:.3e}")
        assert abs(s - r) <= bound
    got = [d.numpy() for d in durs]
    acc = R.frame_accuracy(ids, got, truth)
    same = sum(np.array_equal(a.numpy(), b) for a, b in zip(al.state_durations, want))
    print(f"S {S} optional {optional}: frame accuracy {acc:.4f}, {same} of {len(got)} utterances' state durations as the oracle's")
    assert acc >= cap
    for x, i, d, sd in zip(feats, ids, durs, al.state_durations):
        assert d.dtype == torch.int64 and int(d.sum()) == x.shape[0]
        assert sd.dtype == torch.int64 and sd.shape == (len(i), S) and torch.equal(sd.sum(1), d)
        assert ((sd >= 1).all(1) | (sd == 0).all(1)).all(), "a token has a frame in every state or in none"
    assert model["states"] == S and model["mean"].shape == model["var"].shape == (V * S, D) and model["mean"].dtype == torch.float64
    assert np.allclose(model["mean"].cpu().numpy(), models[-1]["mean"], atol=1e-9) and np.allclose(model["var"].cpu().numpy(), models[-1]["var"], atol=1e-9)


def _bits(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).view(torch.int64)


def _check_scores(what, v, want, got):
    """tests/test_align_scores_kernels_gpu.py's rules: want = R.scores of one utterance, got = the kernel's slices of it."""
    assert np.array_equal(got["amax"], want["amax"]), f"{what}: amax"
    assert torch.equal(_bits(got["margin"]), _bits(want["margin"])), f"{what}: margin bits"
    assert np.array_equal(got["hits"], want["hits"]), f"{what}: hits"
    assert torch.equal(_bits(got["gop_sum"]), _bits(want["gop_sum"])), f"{what}: gop_sum bits"
    assert torch.equal(_bits(got["utt_gop"]), _bits(want["gop_total"])), f"{what}: the utterance's gop bits"
    assert int(got["utt_hits"]) == want["hits_total"], f"{what}: the utterance's hits"
    e = (2 * v + 3 * ((v + 15) // 16 - 1) + 20) * U + 2 * U * np.abs(want["lpost"])
    al, first, total = np.abs(want["lpost"]), 0, 0.0
    assert (np.abs(got["lpost"] - want["lpost"]) <= 2 * e).all(), f"{what}: lpost per frame"
    for p, n in enumerate(want["frames"].tolist()):
        if n == 0:
            assert got["gop_sum"][p] == 0.0 and got["lpost_sum"][p] == 0.0 and got["hits"][p] == 0, f"{what}: token {p} has no frames"
            continue
        b = e[first:first + n].sum() + 2 * (n - 1) * U * al[first:first + n].sum()
        assert abs(got["lpost_sum"][p] - want["lpost_sum"][p]) <= 2 * b, f"{what}: lpost_sum of token {p}"
        first, total = first + n, total + b
    total += 2 * (len(want["frames"]) - 1) * U * np.abs(want["lpost_sum"]).sum()
    assert abs(float(got["utt_lpost"]) - want["lpost_total"]) <= 2 * total, f"{what}: the utterance's lpost"


def test_scores_of_a_two_state_model_are_the_oracles_on_phone_max(gpu):
    S, Vp, Dd = 2, 21, 10
    g = torch.Generator().manual_seed(12)
    al = gpu(n_classes=Vp, states=S)
    model = {"mean": torch.randn(Vp * S, Dd, generator=g, dtype=torch.float64), "var": torch.rand(Vp * S, Dd, generator=g, dtype=torch.float64) * 1.5 + 0.5,
             "states": S}
    shapes = [(1, 2), (1, 9), (3, 6), (17, 40), (5, 9), (65, 200)]           # (5, 9): 5 tokens of 2 states on 9 frames do not fit
    ids = [torch.randint(1, Vp, (P,), generator=g) for P, _ in shapes]
    ids[3][1:16:3] = 0
    feats = [torch.randn(T, Dd, generator=g) * 1.5 for _, T in shapes]
    run = al.run_packed(None, ids, (0,), model, feats=feats)
    sc = al.score_packed(run)
    torch.cuda.synchronize()
    L = run["L"].cpu().numpy().astype(np.float64)
    assert L.shape[0] == Vp * S and sc["phone_L"].shape[0] == Vp
    assert np.array_equal(sc["phone_L"].cpu().numpy().astype(np.float64), R.phone_max(L, S)), "the maximum over the states is exact"
    label, dur, sdur = run["label"].cpu().numpy(), run["durations"].cpu().numpy().astype(np.int64), run["state_durations"].cpu().numpy()
    assert np.array_equal(run["phone_label"].cpu().numpy(), np.where(label < 0, -1, label // S))
    host = {k: v.cpu().numpy() for k, v in sc.items()}
    recs = al.score(None, ids, (0,), model, feats=feats)
    for n, (P, T) in enumerate(shapes):
        f, p = slice(run["foff_host"][n], run["foff_host"][n + 1]), slice(run["poff_host"][n], run["poff_host"][n + 1])
        ok = float(run["score"][n]) > -math.inf
        assert ok == (n != 4) == recs[n]["feasible"]
        if ok:
            assert np.array_equal(label[f], R.state_labels(ids[n].numpy(), sdur[p], S)) and np.array_equal(sdur[p].sum(1), dur[p])
        want = R.scores(R.phone_max(L[:, f], S), ids[n].numpy(), dur[p] if ok else None)
        got = {"margin": host["margin"][f], "lpost": host["lpost"][f], "amax": host["amax"][f], "gop_sum": host["gop_sum"][p],
               "lpost_sum": host["lpost_sum"][p], "hits": host["hits"][p], "utt_gop": host["utt_gop"][n], "utt_lpost": host["utt_lpost"][n],
               "utt_hits": host["utt_hits"][n]}
        _check_scores(f"utterance {n} ({P} x {T})", Vp, want, got)
        if ok:
            assert recs[n]["gop"] == want["gop_total"] / T and recs[n]["phone_acc"] == want["hits_total"] / T
            assert torch.equal(recs[n]["state_durations"], torch.from_numpy(sdur[p]).long()) and torch.equal(recs[n]["durations"], torch.from_numpy(dur[p]))
        else:
            assert recs[n]["state_durations"] is None and recs[n]["durations"] is None and recs[n]["gop"] is None


def test_save_and_load_keep_the_states_and_name_a_mismatch(gpu, tmp_path):
    feats, ids, _, _, _, _ = R.synthetic_corpus_parts(1, 2, n_utts=8)
    ids, feats = [torch.from_numpy(i) for i in ids], [torch.from_numpy(x) for x in feats]
    al = gpu(n_classes=V, states=2)
    model, durs, _ = al.fit(None, ids, feats=feats, iters=2)
    al.save(model, str(tmp_path / "m2.pt"))
    saved = torch.load(tmp_path / "m2.pt", weights_only=True)
    assert set(saved) == {"mean", "var", "K", "n_classes", "states"} and saved["states"] == 2 and saved["n_classes"] == V
    assert saved["mean"].shape == (2 * V, D) and gpu.file_states(str(tmp_path / "m2.pt")) == 2
    loaded = gpu(n_classes=V, states=2).load(str(tmp_path / "m2.pt"))
    assert loaded["states"] == 2
    a, b = al.align(None, ids, (), model, feats=feats), al.align(None, ids, (), loaded, feats=feats)
    for x, y, d, sd in zip(a, b, durs, al.state_durations):
        assert x["feasible"] and x["score"] == y["score"] and torch.equal(x["durations"], y["durations"]) and torch.equal(x["durations"], d)
        assert torch.equal(x["state_durations"], y["state_durations"]) and torch.equal(x["state_durations"], sd)
    with pytest.raises(ValueError, match="a model of states = 2; this aligner has states = 1"):
        gpu(n_classes=V).load(str(tmp_path / "m2.pt"))
    with pytest.raises(ValueError, match="a model of states = 2; this aligner has states = 3"):
        gpu(n_classes=V, states=3).load(str(tmp_path / "m2.pt"))
    with pytest.raises(ValueError, match="the model has states = 2; this aligner has states = 1"):
        gpu(n_classes=V).align(None, ids, (), model, feats=feats)
    # a file without the field is a 1-state model
    one = gpu(n_classes=V)
    m1, d1, _ = one.fit(None, ids, feats=feats, iters=2)
    one.save(m1, str(tmp_path / "m1.pt"))
    assert "states" not in torch.load(tmp_path / "m1.pt", weights_only=True) and gpu.file_states(str(tmp_path / "m1.pt")) == 1
    l1 = gpu(n_classes=V).load(str(tmp_path / "m1.pt"))
    assert "states" not in l1 and all(torch.equal(r["durations"], d) and "state_durations" not in r
                                      for r, d in zip(one.align(None, ids, (), l1, feats=feats), d1))
    with pytest.raises(ValueError, match="a model of states = 1; this aligner has states = 2"):
        al.load(str(tmp_path / "m1.pt"))
    # a file whose class count does not fit its states
    torch.save({**saved, "mean": saved["mean"][:V], "var": saved["var"][:V]}, tmp_path / "bad.pt")
    with pytest.raises(ValueError, match=f"a model of {V} Gaussians; {V} classes of 2 states need {2 * V}"):
        al.load(str(tmp_path / "bad.pt"))


def test_the_limits_raise_by_name_before_any_launch(gpu):
    from kokoro_ruslan_amd import lib as kk
    before = kk.launches
    with pytest.raises(ValueError, match="states must be an integer in 1..3"):
        gpu(states=4)
    with pytest.raises(ValueError, match="states must be an integer in 1..3"):
        gpu(states=0)
    with pytest.raises(ValueError, match="100 phoneme ids of 3 states are 300 classes; at most 256"):
        gpu(n_classes=100, states=3)
    assert gpu(n_classes=59, states=3).classes == 177 and gpu(n_classes=128, states=2).classes == 256
    al = gpu(n_classes=V, states=3)
    with pytest.raises(ValueError, match="the model's mean"):
        al.align(None, [torch.ones(2, dtype=torch.long)], (), {"mean": torch.zeros(V, D), "var": torch.ones(V, D), "states": 3}, feats=[torch.zeros(9, D)])
    with pytest.raises(ValueError, match="1025 tokens"):
        al.fit([torch.zeros(4000, 80)], [torch.ones(1025, dtype=torch.long)])
    assert kk.launches == before


def _entry(g, name, T, P):
    from kokoro.data import features as DF
    ids = torch.randint(1, 59, (P,), generator=g)
    mel = torch.randn(59, 80, generator=g)[torch.repeat_interleave(ids, torch.from_numpy(R.even_split(P, T)))] + 0.3 * torch.randn(T, 80, generator=g)
    ft = {"mel_spec": mel.t().contiguous(), "pitch": torch.rand(T, generator=g), "energy": torch.rand(T, generator=g), "mel_length": T}
    return DF.cache_entry(ft, name, ids, None, None, "text " + name)


def test_kokoro_align_states_on_a_temporary_cache(gpu, tmp_path, capsys):
    from kokoro.cli import align as cli
    from kokoro.data import features as DF
    g = torch.Generator().manual_seed(4)
    cache = tmp_path / "cache"
    shapes = {"u0": (12, 3), "u1": (30, 7), "u2": (42, 21), "u3": (17, 1), "u4": (40, 16), "u5": (25, 6)}
    for name, (T, P) in shapes.items():
        DF.write_cache_entry(str(cache), _entry(g, name, T, P))
    # without --states: the lines and the model file are what they always were, and --states 1 is the same run
    out0, out1, m0, m1 = tmp_path / "d0.jsonl", tmp_path / "d1.jsonl", tmp_path / "m0.pt", tmp_path / "m1.pt"
    assert cli.main(["--cache-dir", str(cache), "--iters", "3", "--batch-size", "4", "--output", str(out0), "--model-out", str(m0)]) == 0
    text0 = capsys.readouterr().out
    assert cli.main(["--cache-dir", str(cache), "--iters", "3", "--batch-size", "4", "--output", str(out1), "--model-out", str(m1), "--states", "1"]) == 0
    assert capsys.readouterr().out == text0 and out0.read_bytes() == out1.read_bytes()
    one = gpu()
    entries = cli.read_cache(str(cache))
    _, durs, _ = one.fit([e["mel"] for e in entries], [e["ids"] for e in entries], iters=3, batch_size=4)
    want = "".join(json.dumps({"name": e["name"], "phoneme_durations": [int(v) for v in d]}) + "\n" for e, d in zip(entries, durs))
    assert out0.read_text() == want, "the default output is the 1-state aligner's, field for field and byte for byte"
    assert set(torch.load(m0, weights_only=True)) == {"mean", "var", "K", "n_classes"}
    # --states 2
    out2, m2 = tmp_path / "d2.jsonl", tmp_path / "m2.pt"
    assert cli.main(["--cache-dir", str(cache), "--iters", "3", "--batch-size", "4", "--output", str(out2), "--model-out", str(m2),
                     "--states", "2", "--write-cache"]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith("kokoro-align: 6 aligned, 0 infeasible (6 utterances), ")
    lines = [json.loads(l) for l in open(out2)]
    assert sorted(l["name"] for l in lines) == sorted(shapes) and all(set(l) == {"name", "phoneme_durations", "state_durations"} for l in lines)
    for l in lines:
        T, P = shapes[l["name"]]
        d, sd = torch.tensor(l["phoneme_durations"]), torch.tensor(l["state_durations"])
        assert sd.shape == (P, 2) and torch.equal(sd.sum(1), d) and int(d.sum()) == T and int(sd.min()) >= 1
        after = torch.load(cache / f"{l['name']}.pt", weights_only=False)
        assert torch.equal(after["phoneme_durations"], d) and after["phoneme_durations"].dtype == torch.long
    assert lines[[l["name"] for l in lines].index("u2")]["state_durations"] == [[1, 1]] * 21
    assert torch.load(m2, weights_only=True)["states"] == 2
    # the file's states hold with --model-in; a conflicting --states is named
    out3 = tmp_path / "d3.jsonl"
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--output", str(out3)]) == 0
    assert [json.loads(l) for l in open(out3)] == lines
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--output", str(out3), "--states", "2"]) == 0
    capsys.readouterr()
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--states", "3"]) == 1
    assert "--states 3" in capsys.readouterr().err
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m0), "--states", "2"]) == 1
    assert "states = 1" in capsys.readouterr().err
    # 9 tokens of 2 states on 17 frames: named, with the flag
    DF.write_cache_entry(str(cache), _entry(g, "short", 17, 9))
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m2), "--output", str(out3)]) == 1
    io = capsys.readouterr()
    assert "short: 9 tokens of 2 states need at least 18 frames and cannot be laid on 17" in io.err and "--states" in io.err
    again = {l["name"]: l for l in map(json.loads, open(out3))}
    assert again["short"]["state_durations"] is None and again["short"]["phoneme_durations"] == R.even_split(9, 17).tolist()
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(m0), "--output", str(out3)]) == 0, "one state per token fits"
