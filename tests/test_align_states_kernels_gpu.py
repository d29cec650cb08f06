"""GPU suite: kk_align_viterbi / kk_align_backtrack (csrc/kk_align.hip), the recurrence and the backtrack of phone models
with S = 1, 2 or 3 states per phoneme, called on a given L [V S, T_total] and held against the fp64 oracle
(kokoro_ruslan_amd.align_torch.viterbi_states).

Shapes: P in {1, 2, 15, 16, 17, 63, 64, 65} (the code word's and the wave's edges), T in {S P, S P + 1, 7, 8, 9, 17, 2 S P + 3} where a
path exists (the eight-frame prefetch's edges), every S, and optional tokens nowhere, inside, first and last.

  parent    every output at every S is, bit for bit, what the entry points of the commit before the two kernel families became one
            gave on the same L (tests/golden/align_parent_outputs.npz, recorded on an MI355X).
  exact     L holds integers in -6..6, so every fp32 sum is exact and the kernel must agree with the oracle in every state duration,
            the score and every label, ties included (there are many).
  random    fp32 near-ties may choose differently, so as in test_align_kernels_gpu.py the score pins the recurrence: with S64 the
            oracle's optimum on the same L and A = sum_t max_c |L(c, t)|, |score - S64| <= T 2^-23 A, and the fp64 score of the
            kernel's own state durations is >= S64 - T 2^-23 A (the derivation stands there; S changes neither the number of terms
            along a path nor their bound).  And the result is a valid path."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import align_torch as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
V = 7
OPT = 0
PS = (1, 2, 15, 16, 17, 63, 64, 65)
STATES = (1, 2, 3)
VARIANTS = ("none", "inner", "first", "last")
PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_parent_outputs.npz")


def _ids(g, P, variant):
    ids = torch.randint(1, V, (P,), generator=g)
    if variant == "inner":
        ids[1:P - 1:3] = OPT
    elif variant == "first":
        ids[0] = OPT
    elif variant == "last":
        ids[P - 1] = OPT
    return ids


def _items(S):
    out = []
    for P in PS:
        for T in sorted({S * P, S * P + 1, 7, 8, 9, 17, 2 * S * P + 3}):
            for var in VARIANTS:
                mandatory = P - len(range(1, P - 1, 3)) if var == "inner" else P - (1 if var in ("first", "last") else 0)
                if T >= S * max(mandatory, 1) and (var == "none" or P > 1):
                    out.append((P, T, var))
    return out


def launch(S, L, ids, frames, threads=None, state_durations=True, out=None):
    """One launch of the Viterbi and the backtrack entry points on L [V S, T_total] for utterances of ids[n] tokens and frames[n]
    frames; without `state_durations` the backtrack gets NULL for them.  Every output on the host, with the offsets.  out: a dict
    that receives the outputs on the device before anything is called (for a call that raises)."""
    from kokoro_ruslan_amd import lib as kk
    from kokoro_ruslan_amd.align import code_words
    dev = "cuda"
    tokens = [int(i.shape[0]) for i in ids]
    B = len(ids)
    tok = torch.cat(ids)
    foff, poff = kk.packed_offsets(frames), kk.packed_offsets(tokens)
    coff = kk.packed_offsets([code_words(p, t, S) for p, t in zip(tokens, frames)])
    assert int(foff[-1]) == L.shape[1] and L.shape[0] == V * S and L.dtype == torch.float32
    d = dict(L=L.to(dev).contiguous(), ids=tok.to(torch.int32).to(dev), opt=(tok == OPT).to(torch.uint8).to(dev),
             foff=foff.to(torch.int32).to(dev), poff=poff.to(torch.int32).to(dev), coff=coff.to(dev))
    threads = threads or (max(tokens) + 63) // 64 * 64
    out = {} if out is None else out
    out.update(score=torch.full((B,), 7.0, device=dev), end=torch.full((B,), 7, dtype=torch.int32, device=dev),
               codes=torch.zeros(int(coff[-1]), dtype=torch.int32, device=dev),
               durations=torch.full((int(poff[-1]),), 7, dtype=torch.int32, device=dev),
               label=torch.full((int(foff[-1]),), 7, dtype=torch.int32, device=dev))
    if state_durations:
        out["state_durations"] = torch.full((int(poff[-1]), S), 7, dtype=torch.int32, device=dev)
    kk.call("kk_align_viterbi", d["L"], L.shape[1], d["ids"], d["opt"], d["foff"], d["poff"], d["coff"], B, threads, S, out["score"],
            out["end"], out["codes"])
    kk.call("kk_align_backtrack", out["codes"], d["coff"], d["foff"], d["poff"], d["ids"], out["end"], B, S, out.get("state_durations"),
            out["durations"], out["label"])
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in out.items()}
    host.update(foff=foff.tolist(), poff=poff.tolist(), coff=coff.tolist())
    return host


def pieces(run, n):
    """Every output of utterance n, as host tensors."""
    f0, f1, p0, p1, c0, c1 = (run[k][n + j] for k in ("foff", "poff", "coff") for j in (0, 1))
    out = {"score": run["score"][n:n + 1], "end": run["end"][n:n + 1], "codes": run["codes"][c0:c1], "durations": run["durations"][p0:p1],
           "label": run["label"][f0:f1]}
    if "state_durations" in run:
        out["state_durations"] = run["state_durations"][p0:p1]
    return out


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    runs = {}

    def get(S, kind):
        """All items of S in one launch, on random fp32 L ("random") or on small integers ("exact"); computed once, never changed."""
        if (S, kind) not in runs:
            g = torch.Generator().manual_seed(100 * S + (kind == "exact"))
            items = _items(S)
            ids = [_ids(g, P, var) for P, _, var in items]
            frames = [T for _, T, _ in items]
            n = sum(frames)
            L = (torch.randint(-6, 7, (V * S, n), generator=g).float() if kind == "exact" else torch.randn(V * S, n, generator=g) * 3.0)
            runs[(S, kind)] = dict(items=items, ids=ids, frames=frames, L=L, run=launch(S, L, ids, frames))
        return runs[(S, kind)]
    return get


def _oracle(w, n, S):
    r = pieces(w["run"], n)
    f0, f1 = w["run"]["foff"][n], w["run"]["foff"][n + 1]
    L = w["L"][:, f0:f1].numpy().astype(np.float64)
    i = w["ids"][n].numpy()
    sd64, pd64, S64 = R.viterbi_states(L, i, S, i == OPT)
    return r, L, i, sd64, pd64, S64


def _sha256(x):
    return hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest()


def test_every_output_is_the_parent_commits_bit_for_bit(world):
    """tests/golden/align_parent_outputs.npz was recorded on an MI355X at the commit it names ("commit"), the last one with a 1-state
    kernel pair beside the S-state pair, by launching that commit's own entry points on this module's world(S, kind) inputs (a job
    script that is not kept: it built the inputs as `world` does and called this module's launch() of that commit).  It holds, for
    world(1, "random") (107 utterances, 4237 frames), L and the full outputs of the 1-state kk_align_viterbi / kk_align_backtrack, which
    that commit's test proved equal to its S-state kernels' at S = 1; and for world(1, "exact") and both kinds at S = 2 and 3 the
    SHA-256 of L and of every output of kk_align_viterbi_states / kk_align_backtrack_states."""
    gold = np.load(PARENT)
    print(f"recorded at {gold['commit']}")
    w = world(1, "random")
    assert same_bits(w["L"], torch.from_numpy(gold["L"])), "the regenerated L of world(1, 'random') is not the L the fixture was recorded on"
    new = launch(1, torch.from_numpy(gold["L"]), w["ids"], w["frames"])
    for k in ("score", "end", "codes", "durations", "label"):
        assert same_bits(new[k], torch.from_numpy(gold[k])), k
        assert same_bits(w["run"][k], new[k]), k
    assert same_bits(new["state_durations"][:, 0], torch.from_numpy(gold["durations"]))
    for S, kind in ((1, "exact"), (2, "random"), (2, "exact"), (3, "random"), (3, "exact")):
        w = world(S, kind)
        assert _sha256(w["L"]) == str(gold[f"sha256_{S}_{kind}_L"]), \
            f"the regenerated L of world({S}, {kind!r}) is not the L the fixture was recorded on"
        for k in ("score", "end", "codes", "state_durations", "durations", "label"):
            assert _sha256(w["run"][k]) == str(gold[f"sha256_{S}_{kind}_{k}"]), (S, kind, k)
    w, new = world(1, "random"), world(1, "random")["run"]
    skipped = sum(int(((pieces(new, n)["durations"] == 0) & (w["ids"][n] == OPT)).sum()) for n in range(len(w["items"])))
    first = sum(int(pieces(new, n)["durations"][0] == 0) for n, it in enumerate(w["items"]) if it[2] == "first")
    last = sum(int(pieces(new, n)["durations"][-1] == 0) for n, it in enumerate(w["items"]) if it[2] == "last")
    print(f"{len(w['items'])} items, {skipped} optional tokens skipped, {first} at position 0, {last} at position P - 1")
    assert skipped > 0 and first > 0 and last > 0


def test_state_durations_may_be_null_with_one_state_only(world):
    w = world(1, "exact")
    bare = launch(1, w["L"], w["ids"], w["frames"], state_durations=False)
    assert "state_durations" not in bare
    for k in ("score", "end", "codes", "durations", "label"):
        assert same_bits(bare[k], w["run"][k]), k
    w = world(2, "exact")
    refused = {}
    with pytest.raises(RuntimeError, match="kk_align_backtrack: 2 states need state_durations"):
        launch(2, w["L"], w["ids"], w["frames"], state_durations=False, out=refused)
    torch.cuda.synchronize()
    assert (refused["durations"] == 7).all() and (refused["label"] == 7).all()      # refused before any launch
    for k in ("score", "end", "codes"):                                   # (the Viterbi launch had run)
        assert same_bits(refused[k].cpu(), w["run"][k]), k


@pytest.mark.parametrize("S", STATES)
def test_exact_integers_equal_the_oracle_ties_included(world, S):
    w = world(S, "exact")
    for n, (P, T, var) in enumerate(w["items"]):
        r, L, i, sd64, pd64, S64 = _oracle(w, n, S)
        assert sd64 is not None, (P, T, var)
        assert float(r["score"]) == S64, (P, T, var)
        assert np.array_equal(r["state_durations"].numpy(), sd64), (P, T, var)
        assert np.array_equal(r["durations"].numpy(), pd64)
        assert np.array_equal(r["label"].numpy(), R.state_labels(i, sd64, S))
        assert int(r["end"]) == (P - 1 if pd64[P - 1] > 0 else P - 2)
        if T == S * P and var == "none":
            assert sd64.tolist() == [[1] * S] * P


@pytest.mark.parametrize("S", STATES)
def test_random_l_scores_the_optimum_on_a_valid_path(world, S):
    w = world(S, "random")
    seen = {v: [0, 0] for v in VARIANTS[1:]}
    for n, (P, T, var) in enumerate(w["items"]):
        r, L, i, sd64, pd64, S64 = _oracle(w, n, S)
        assert sd64 is not None
        sd, d, opt = r["state_durations"].numpy().astype(np.int64), r["durations"].numpy().astype(np.int64), i == OPT
        bound = T * EPS * float(np.abs(L).max(0).sum())
        assert int(sd.min()) >= 0 and int(sd.sum()) == T, "the state durations sum to T"
        assert np.array_equal(d, sd.sum(1)), "the phone durations are the row sums"
        present = d > 0
        assert (sd[present] >= 1).all(), "every state of a present token has a frame"
        assert not (~present & ~opt).any(), "only an optional token may get no frame"
        assert not (~present[1:] & ~present[:-1]).any(), "two adjacent tokens are never both skipped"
        assert np.array_equal(r["label"].numpy(), R.state_labels(i, sd, S)), "label is the class of every frame's state"
        assert int(r["end"]) == (P - 1 if d[P - 1] > 0 else P - 2)
        got, score = R.path_score_states(L, i, sd, S), float(r["score"])
        if n % 16 == 0:
            print(f"S {S} item {P} x {T} ({var}): score {score!r}  S64 {S64!r}  |difference| {abs(score - S64):.3e}  "
                  f"S64 - the fp64 score of the kernel's path {S64 - got:.3e}  bound {bound:.3e}")
        assert abs(score - S64) <= bound, (P, T, var)
        assert got >= S64 - bound, (P, T, var)
        if var != "none":
            seen[var][0] += int((~present).sum())
            seen[var][1] += int((present & opt).sum())
    print(seen)
    for var, (skipped, kept) in seen.items():
        assert skipped > 0 and kept > 0, f"{var}: {skipped} skipped, {kept} kept"


@pytest.mark.parametrize("S", STATES)
def test_one_frame_too_few_is_infeasible_and_disturbs_no_neighbour(world, S):
    g = torch.Generator().manual_seed(40 + S)
    ids = [_ids(g, 5, "none"), _ids(g, 9, "inner"), _ids(g, 17, "none"), _ids(g, 2, "first"), _ids(g, 5, "none")]
    mandatory = [int((i != OPT).sum()) for i in ids]
    frames = [S * 5 + 4, S * mandatory[1] - 1, S * 17 - 1, max(S * mandatory[3] - 1, 1), S * 5 + 4]
    if S == 1:                                                            # (one mandatory token of one state: T = 0 does not exist)
        ids, frames, mandatory = ids[:3] + ids[4:], frames[:3] + frames[4:], mandatory[:3] + mandatory[4:]
    L = torch.randn(V * S, sum(frames), generator=g)
    run = launch(S, L, ids, frames)
    for n in range(len(ids)):
        r = pieces(run, n)
        if frames[n] < S * mandatory[n]:
            assert float(r["score"]) == -math.inf and int(r["end"]) == -1
            assert not r["state_durations"].any() and not r["durations"].any() and (r["label"] == -1).all()
        else:
            alone = pieces(launch(S, L[:, run["foff"][n]:run["foff"][n + 1]], [ids[n]], [frames[n]]), 0)
            assert int(r["durations"].sum()) == frames[n]
            for k in r:
                assert same_bits(r[k], alone[k]), k
    assert sum(f < S * m for f, m in zip(frames, mandatory)) >= 2


def test_the_largest_shape_gives_all_ones(world):
    from kokoro_ruslan_amd import align as A
    P = A.max_tokens()
    assert P == 1024
    g = torch.Generator().manual_seed(2)
    L, ids = torch.randn(V * 3, 3 * P, generator=g), _ids(g, P, "none")
    run = launch(3, L, [ids], [3 * P])
    assert (run["state_durations"] == 1).all() and (run["durations"] == 3).all() and int(run["end"]) == P - 1
    want = R.state_labels(ids.numpy(), np.ones((P, 3), dtype=np.int64), 3)
    assert np.array_equal(run["label"].numpy(), want)
    S64 = float(L.numpy().astype(np.float64)[want, np.arange(3 * P)].sum())  # the only path
    assert abs(float(run["score"]) - S64) <= 3 * P * EPS * float(L.abs().max(0).values.double().sum())


@pytest.mark.parametrize("S", STATES)
def test_an_utterances_outputs_do_not_depend_on_the_batch(world, S):
    g = torch.Generator().manual_seed(60 + S)
    shapes = [(17, 17 * S + 20, "inner"), (130, 130 * S + 41, "inner"), (5, 5 * S - 1, "none"), (64, 64 * S + 9, "last")]
    ids = [_ids(g, P, var) for P, _, var in shapes]
    frames = [T for _, T, _ in shapes]
    Ls = [torch.randn(V * S, T, generator=g) * 3.0 for T in frames]

    def batch(order, threads=None):
        return launch(S, torch.cat([Ls[n] for n in order], 1), [ids[n] for n in order], [frames[n] for n in order], threads)
    for n in range(len(shapes)):
        others = [m for m in range(len(shapes)) if m != n]
        alone = pieces(batch([n]), 0)                                     # at its own workgroup size
        feasible = frames[n] >= S * int((ids[n] != OPT).sum())
        assert (int(alone["end"]) >= 0) == feasible
        for order, at, threads in (([n], 0, 192), ([n] + others, 0, None), (others + [n], len(others), None),
                                   (others[:1] + [n] + others[1:], 1, None), ([n] + others, 0, 1024)):
            got = pieces(batch(order, threads), at)
            for k in alone:
                assert same_bits(alone[k], got[k]), f"S {S} utterance {n} in {order} at {threads} threads: {k} differs"
