"""GPU suite: after kk_align_loglik became the one likelihood entry point (M = 1, 2 or 4 components), the dense and the list
statistics kernels one core, the block scans one and `PhoneAligner.fit`'s passes one loop, every public result is, bit for bit, what the
commit before gave (tests/golden/align_parent_mix_outputs.npz, recorded on an MI355X by tools/record_align_golden.py at that commit).

`outputs()` below is the whole case list.  It uses only `PhoneAligner`'s public methods, whose signatures did not change, so the same
function ran at the parent commit and runs here; every input is seeded and generated on the CPU.  The fixture holds the SHA-256 of
every result and the small ones also as they are; it is the memory of what the kernels gave, so a change meant to keep their bits never
regenerates it.

  loglik          C = 59 (the last workgroup of 16 / M classes is partial at every M), T = 300 (a full workgroup of frames and a
                  partial one), M in {1, 2, 4}, D in {2, 8, 9, 32, 33, 64} (both sides of the kernels' 8 / 32 / 64 registers), one weight
                  of 0 at M > 1 (a component of -inf).  And at M = 1 the d in {2, 28, 64} cases, seeds and all, that used to be held
                  against the single-Gaussian entry point when there were two.
  accumulate      the labels of test_align_mix_kernels_gpu.py (an empty class, a one-frame class, -1 frames, a label past the model), G in
                  {2, 59, 256}, D in {2, 5, 28, 64} (2 and 5: a partial last group of four dimensions), T in {1, 255, 256, 257, 5000}.
  accumulate_mix  the same, and G in {300, 1024}.
  score           one batch: P = 1 and T = 1; P = 1024 and T = 2048 (every thread owns four tokens, all four waves live); P = 100 and T
                  = 37 (most durations 0); an infeasible utterance (durations 0, labels -1).  V = 59, L random fp32.
  fit             align_torch.synthetic_corpus_modes(0), iters = 4, mix_iters = 2, batch_size = 16, (states, mixtures) in {(1, 1), (2,
                  1), (1, 2), (2, 4)}: the model, every duration and state duration, the scores, and the model's keys."""
import hashlib
import os
from typing import Dict

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R
from test_align_mix_kernels_gpu import _labels, _model

pytestmark = pytest.mark.gpu

PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_parent_mix_outputs.npz")
RAW_BYTES = 512                          # a result up to this size is also stored as it is, beside its SHA-256
C, T_LL, V_SC = 59, 300, 59
FITS = ((1, 1), (2, 1), (1, 2), (2, 4))


def _loglik(A, out):
    for m in (1, 2, 4):
        al = A.PhoneAligner(n_classes=C, mixtures=m)
        for d in (2, 8, 9, 32, 33, 64):
            g = torch.Generator().manual_seed(1000 * m + d)
            feat = (torch.randn(d, T_LL, generator=g) * 1.5).cuda().contiguous()
            model = _model(g, C, m, d)
            if m > 1:
                model["weight"][3, 1] = 0.0
            out[f"loglik/M{m}_D{d}"] = al.loglik(feat, model)
    al = A.PhoneAligner(n_classes=C)
    for d in (2, 28, 64):                                                        # (the seeds of the test this file replaced)
        g = torch.Generator().manual_seed(d)
        feat = (torch.randn(d, T_LL, generator=g) * 1.5).cuda().contiguous()
        out[f"loglik/single_D{d}"] = al.loglik(feat, _model(g, C, 1, d))


def _accumulate(A, out):
    for G in (2, 59, 256, 300, 1024):
        al = A.PhoneAligner(n_classes=min(G, 256))
        for D in (2, 5, 28, 64):
            for T in (1, 255, 256, 257, 5000):
                g = torch.Generator().manual_seed(G + D + T)
                feat = (torch.randn(D, T, generator=g) * 3.0 + 1.0).cuda().contiguous()
                lab = _labels(g, G, T).cuda()
                if G <= 256:
                    for k, x in zip(("count", "sum", "sumsq"), al.accumulate(feat, lab)):
                        out[f"accumulate/G{G}_D{D}_T{T}_{k}"] = x
                for k, x in zip(("count", "sum", "sumsq"), al.accumulate_mix(feat, lab, G)):
                    out[f"accumulate_mix/G{G}_D{D}_T{T}_{k}"] = x


def _score(A, out):
    g = torch.Generator().manual_seed(5)
    tokens, frames = (1, 1024, 100, 50), (1, 2048, 37, 20)
    ids = [torch.randint(0, V_SC, (p,), generator=g) for p in tokens]
    dur = [torch.ones(1, dtype=torch.long),
           torch.ones(1024, dtype=torch.long) + torch.bincount(torch.randint(0, 1024, (1024,), generator=g), minlength=1024),
           torch.bincount(torch.randint(0, 100, (37,), generator=g), minlength=100),      # optional tokens: most have no frame
           torch.zeros(50, dtype=torch.long)]                                             # infeasible: 50 tokens, 20 frames
    label = [torch.repeat_interleave(i, d) for i, d in zip(ids[:3], dur[:3])] + [torch.full((20,), -1, dtype=torch.long)]
    assert [int(d.sum()) for d in dur[:3]] == list(frames[:3]) and (dur[2] == 0).sum() > 50
    foff, poff = np.cumsum((0,) + frames).tolist(), np.cumsum((0,) + tokens).tolist()
    dev = lambda x: x.to(torch.int32).cuda()
    run = {"L": (torch.randn(V_SC, foff[-1], generator=g) * 4.0 - 20.0).cuda(), "label": dev(torch.cat(label)), "durations": dev(torch.cat(dur)),
           "ids": dev(torch.cat(ids)), "foff": dev(torch.tensor(foff)), "poff": dev(torch.tensor(poff)), "foff_host": foff, "poff_host": poff}
    for k, x in A.PhoneAligner(n_classes=V_SC).score_packed(run).items():
        out[f"score/{k}"] = x


def _fit(A, out):
    feats, ids, _, _, _, _ = R.synthetic_corpus_modes(0)
    feats, ids = [torch.from_numpy(f) for f in feats], [torch.from_numpy(i) for i in ids]
    for S, M in FITS:
        al = A.PhoneAligner(K=3, n_classes=12, states=S, mixtures=M)
        model, durs, scores = al.fit(None, ids, (), iters=4, mix_iters=2, batch_size=16, feats=feats)
        assert all(d is not None for d in durs)
        pre = f"fit/S{S}_M{M}_"
        for k in ("mean", "var", "weight"):
            if k in model:
                out[pre + k] = model[k]
        out[pre + "durations"] = torch.cat(durs)
        if S > 1:
            out[pre + "state_durations"] = torch.cat(al.state_durations)
        out[pre + "scores"] = torch.tensor(scores, dtype=torch.float64)
        out[pre + "keys"] = " ".join(sorted(model))


def outputs() -> Dict:
    """name -> tensor on the host (or a string), in a fixed order."""
    from kokoro_ruslan_amd import align as A
    out: Dict = {}
    for part in (_loglik, _accumulate, _score, _fit):
        part(A, out)
    return {k: x if isinstance(x, str) else x.detach().cpu().contiguous() for k, x in out.items()}


def digest(x) -> str:
    if isinstance(x, str):
        return hashlib.sha256(x.encode()).hexdigest()
    a = x.numpy()
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def fixture_of(new: Dict, commit: str) -> Dict:
    """The arrays of the fixture: "names" and the SHA-256 of every result beside them; the small results also as they are."""
    out = {"commit": np.array(commit), "names": np.array(list(new)), "sha256": np.array([digest(x) for x in new.values()])}
    out.update({k: np.array(x) if isinstance(x, str) else x.numpy() for k, x in new.items() if isinstance(x, str) or x.numpy().nbytes <= RAW_BYTES})
    return out


@pytest.fixture(scope="module")
def both():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    gold = np.load(PARENT)
    print(f"recorded at {gold['commit']}")
    return gold, outputs()


def test_the_recorded_results_are_the_case_list(both):
    gold, new = both
    assert gold["names"].tolist() == list(new)
    count = lambda part: sum(k.startswith(part + "/") for k in new)
    assert count("loglik") == 21 and count("accumulate") == 180 and count("accumulate_mix") == 300 and count("score") == 9
    assert count("fit") == sum(5 + (S > 1) + (M > 1) for S, M in FITS)
    raw = set(gold.files) - {"commit", "names", "sha256"}
    assert raw == set(fixture_of(new, "")) - {"commit", "names", "sha256"} and len(raw) >= 60


@pytest.mark.parametrize("part", ["loglik", "accumulate", "accumulate_mix", "score", "fit"])
def test_every_result_is_the_parent_commits_bit_for_bit(both, part):
    gold, new = both
    want = dict(zip(gold["names"].tolist(), gold["sha256"].tolist()))
    for k, x in new.items():
        if k.startswith(part + "/"):
            if k in gold.files and not isinstance(x, str):                       # a small one: say where it differs
                assert np.array_equal(gold[k].view(np.uint8), x.numpy().view(np.uint8)), (k, gold[k], x)
            assert digest(x) == want[k], k


def test_a_model_says_states_and_mixtures_only_when_there_are_several(both):
    _, new = both
    for S, M in FITS:
        keys = ["K", "mean"] + ["mixtures"] * (M > 1) + ["n_classes"] + ["states"] * (S > 1) + ["var"] + ["weight"] * (M > 1)
        assert new[f"fit/S{S}_M{M}_keys"] == " ".join(keys)
