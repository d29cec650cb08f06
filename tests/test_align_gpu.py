"""GPU suite: PhoneAligner.fit (Viterbi training on the device) against the fp64 oracle's fit on a synthetic corpus with a known
alignment, the model's save / load round trip, and the kokoro-align tool on a temporary feature cache.

The corpus is align_torch.synthetic_corpus(0), passed as features.  Per pass the device's corpus score must lie within the summed kernel
bound of the oracle's: per utterance T 2^-23 A for the recurrence (test_align_kernels_gpu.py derives it) plus, per frame, the largest
distance of the fp32 log-likelihood from the fp64 one: (D + 8) 2^-23 E(v, t), E = sum_d |a| (|x| + |mu|)^2 + |c|: the chain's (D + 4)
roundings on terms bounded by E, and four more units for the rounding of a, mu and c to fp32 (2 u |a| |x - mu| |mu| <= 2 u E for mu, u E
each for a and c), all doubled."""
import json
import math

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
V, D = 12, 8


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


@pytest.mark.parametrize("optional,cap", [(False, 0.99), (True, 0.97)])
def test_fit_follows_the_oracle_pass_by_pass(gpu, optional, cap):
    feats, ids, opts, truth, _ = R.synthetic_corpus(0, optional)
    models = []
    _, want, ref_scores = R.fit(feats, ids, opts if optional else None, V=V, models=models)
    al = gpu(n_classes=V)
    model, durs, scores = al.fit(None, [torch.from_numpy(i) for i in ids], (0,) if optional else (), batch_size=16,
                                 feats=[torch.from_numpy(x) for x in feats])
    assert len(scores) == len(ref_scores) < 6, (scores, ref_scores)
    for n, (s, r, m) in enumerate(zip(scores, ref_scores, models)):
        bound = _pass_bound(feats, m)
        print(f"optional {optional} pass {n}: device {s!r}  oracle {r!r}  |difference| {abs(s - r):.3e}  bound {bound:.3e}")
        assert abs(s - r) <= bound
    got = [d.numpy() for d in durs]
    acc = R.frame_accuracy(ids, got, truth)
    print(f"optional {optional}: frame accuracy {acc:.4f}, {sum(np.array_equal(a, b) for a, b in zip(got, want))} of {len(got)} utterances as the oracle")
    assert acc >= cap
    for x, d in zip(feats, durs):
        assert d.dtype == torch.int64 and int(d.sum()) == x.shape[0]
    assert model["mean"].shape == model["var"].shape == (V, D) and model["mean"].dtype == torch.float64
    assert np.allclose(model["mean"].cpu().numpy(), models[-1]["mean"], atol=1e-9) and np.allclose(model["var"].cpu().numpy(), models[-1]["var"], atol=1e-9)


def test_save_and_load_give_identical_durations(gpu, tmp_path):
    feats, ids, _, _, _ = R.synthetic_corpus(1, False, n_utts=8)
    al = gpu(n_classes=V)
    ids, feats = [torch.from_numpy(i) for i in ids], [torch.from_numpy(x) for x in feats]
    model, durs, _ = al.fit(None, ids, feats=feats, iters=2)
    al.save(model, str(tmp_path / "m.pt"))
    saved = torch.load(tmp_path / "m.pt", weights_only=True)
    assert set(saved) == {"mean", "var", "K", "n_classes"} and saved["K"] == 13 and saved["n_classes"] == V
    loaded = gpu(n_classes=V).load(str(tmp_path / "m.pt"))
    a, b = al.align(None, ids, (), model, feats=feats), al.align(None, ids, (), loaded, feats=feats)
    for x, y, d in zip(a, b, durs):
        assert x["feasible"] and x["score"] == y["score"] and torch.equal(x["durations"], y["durations"]) and torch.equal(x["durations"], d)
    with pytest.raises(ValueError, match="a model of K = 13, 12 classes"):
        gpu(n_classes=V + 1).load(str(tmp_path / "m.pt"))


def _entry(g, name, T, P):
    from kokoro.data import features as DF
    ids = torch.randint(1, 59, (P,), generator=g)
    mel = torch.randn(59, 80, generator=g)[torch.repeat_interleave(ids, torch.from_numpy(R.even_split(P, T)))] + 0.3 * torch.randn(T, 80, generator=g)
    ft = {"mel_spec": mel.t().contiguous(), "pitch": torch.rand(T, generator=g), "energy": torch.rand(T, generator=g), "mel_length": T}
    return DF.cache_entry(ft, name, ids, None, None, "text " + name)


def _same(a, b, but=()):
    assert set(a) == set(b)
    for k, v in a.items():
        if k not in but:
            assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k


def test_kokoro_align_on_a_temporary_cache(gpu, tmp_path, capsys):
    from kokoro.cli import align as cli
    from kokoro.data import features as DF
    from kokoro.data.cached import reference_reconcile
    g = torch.Generator().manual_seed(4)
    cache = tmp_path / "cache"
    shapes = {"u0": (12, 3), "u1": (30, 7), "u2": (21, 21), "u3": (17, 1), "u4": (40, 16), "u5": (25, 6)}
    for name, (T, P) in shapes.items():
        DF.write_cache_entry(str(cache), _entry(g, name, T, P))
    before = {n: torch.load(cache / f"{n}.pt", weights_only=False) for n in shapes}
    out, model = tmp_path / "d.jsonl", tmp_path / "m.pt"
    assert cli.main(["--cache-dir", str(cache), "--iters", "3", "--batch-size", "4", "--output", str(out), "--model-out", str(model),
                     "--write-cache"]) == 0
    summary = capsys.readouterr().out.strip().splitlines()[-1]
    assert summary.startswith("kokoro-align: 6 aligned, 0 infeasible (6 utterances), ") and "passes" in summary
    lines = [json.loads(l) for l in open(out)]
    assert sorted(l["name"] for l in lines) == sorted(shapes) and all(set(l) == {"name", "phoneme_durations"} for l in lines)
    for l in lines:
        T, P = shapes[l["name"]]
        d = torch.tensor(l["phoneme_durations"])
        assert d.shape == (P,) and int(d.sum()) == T and int(d.min()) >= 1
        assert torch.equal(reference_reconcile(d, T), d), "the durations sum to mel_length: the reference's reconciliation is the identity"
        after = torch.load(cache / f"{l['name']}.pt", weights_only=False)
        _same(before[l["name"]], after, but=("phoneme_durations",))
        assert torch.equal(after["phoneme_durations"], d) and after["phoneme_durations"].dtype == torch.long
    assert lines[[l["name"] for l in lines].index("u2")]["phoneme_durations"] == [1] * 21
    assert sorted(f.name for f in cache.glob("*.pt*")) == sorted(f"{n}.pt" for n in shapes)
    # a second run that loads the model reproduces the durations
    out2 = tmp_path / "d2.jsonl"
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(model), "--output", str(out2)]) == 0
    assert [json.loads(l) for l in open(out2)] == lines
    # an entry with more tokens than frames stays as it is, is reported, and makes the exit status 1
    DF.write_cache_entry(str(cache), _entry(g, "bad", 4, 9))
    raw = (cache / "bad.pt").read_bytes()
    capsys.readouterr()
    assert cli.main(["--cache-dir", str(cache), "--model-in", str(model), "--output", str(out2), "--write-cache"]) == 1
    io = capsys.readouterr()
    assert "bad: 9 tokens cannot be laid on 4 frames" in io.err
    assert io.out.strip().splitlines()[-1].startswith("kokoro-align: 6 aligned, 1 infeasible (7 utterances), ")
    assert (cache / "bad.pt").read_bytes() == raw
    again = {l["name"]: l["phoneme_durations"] for l in map(json.loads, open(out2))}
    assert again["bad"] == _entry(g, "bad", 4, 9)["phoneme_durations"].tolist() == R.even_split(9, 4).tolist()
    assert all(again[l["name"]] == l["phoneme_durations"] for l in lines)
    assert math.isfinite(float(io.out.strip().splitlines()[-1].split("per frame ")[1].split()[0]))
