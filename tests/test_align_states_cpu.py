"""CPU suite: the fp64 oracle of the multi-state phone models (kokoro_ruslan_amd.align_torch.viterbi_states and what stands around it):
S = 1 is `viterbi`, tiny cases against a brute-force enumeration of every valid state path, feasibility, the one-frame-per-state case,
features at the class means, and what the feature is for: on phones that are not stationary a 2-state model aligns better."""
import itertools
import math

import numpy as np
import pytest

from kokoro_ruslan_amd import align_torch as R


def _rand_L(g, C, T):
    return g.normal(0.0, 3.0, (C, T))


@pytest.mark.parametrize("seed", range(6))
def test_one_state_is_viterbi(seed):
    g = np.random.default_rng(seed)
    for P, T in ((1, 1), (1, 5), (3, 3), (4, 9), (7, 30), (12, 11), (6, 5)):
        V = 9
        L = _rand_L(g, V, T)
        ids = g.integers(1, V, P)
        for with_opt in (False, True):
            opt = None
            if with_opt:
                opt = g.random(P) < 0.4
                ids = np.where(opt, 0, ids)
            d, s = R.align(L, ids, opt)
            sd, pd, ss = R.viterbi_states(L, ids, 1, opt)
            if d is None:
                assert sd is None and pd is None and ss == -math.inf and s == -math.inf
                continue
            assert ss == s and np.array_equal(pd, d) and sd.shape == (P, 1) and np.array_equal(sd[:, 0], d)
            assert np.array_equal(R.state_labels(ids, sd, 1), np.repeat(ids, d))
            assert R.path_score_states(L, ids, sd, 1) == R.path_score(L, ids, d)


def _valid_paths(P, T, S, opt):
    """Every valid state-duration matrix [P, S]: a present token has >= 1 frame in every state, an absent one (only an optional one,
    never two adjacent) has none, all sum to T."""
    for present in itertools.product((False, True), repeat=P):
        if any(not present[p] and not opt[p] for p in range(P)) or any(not present[p] and not present[p + 1] for p in range(P - 1)):
            continue
        n = S * sum(present)
        if n < 1 or n > T:
            continue
        cells = [(p, j) for p in range(P) if present[p] for j in range(S)]
        for cuts in itertools.combinations(range(1, T), n - 1):                  # compositions of T into n positive parts
            parts = np.diff((0,) + cuts + (T,))
            sd = np.zeros((P, S), dtype=np.int64)
            for (p, j), d in zip(cells, parts):
                sd[p, j] = d
            yield sd


CASES = [(P, T, S, opt) for S in (2, 3) for P in (1, 2, 3, 4) for T in range(1, 10)
         for opt in itertools.product((False, True), repeat=P)]


def test_brute_force_has_the_oracles_optimum_and_feasibility():
    g = np.random.default_rng(7)
    seen = {"feasible": 0, "infeasible": 0, "skipped": 0}
    for P, T, S, opt in CASES:
        V = 5
        ids = np.where(np.array(opt), 0, g.integers(1, V, P))
        L = _rand_L(g, V * S, T)
        best = max((R.path_score_states(L, ids, sd, S) for sd in _valid_paths(P, T, S, opt)), default=None)
        sd, pd, score = R.viterbi_states(L, ids, S, np.array(opt))
        if best is None:
            seen["infeasible"] += 1
            assert sd is None and pd is None and score == -math.inf, (P, T, S, opt)
            continue
        seen["feasible"] += 1
        assert sd is not None, (P, T, S, opt)
        assert any(np.array_equal(sd, v) for v in _valid_paths(P, T, S, opt)), "the oracle's path must be a valid one"
        assert np.array_equal(pd, sd.sum(1)) and int(pd.sum()) == T
        assert score == pytest.approx(best, rel=1e-12, abs=1e-12)
        assert R.path_score_states(L, ids, sd, S) == pytest.approx(score, rel=1e-12, abs=1e-12)
        seen["skipped"] += int((pd == 0).sum())
    print(seen)
    assert min(seen.values()) > 20


@pytest.mark.parametrize("S", [1, 2, 3])
def test_infeasible_exactly_below_s_times_the_mandatory_tokens(S):
    g = np.random.default_rng(S)
    ids = np.array([1, 0, 2, 3, 0, 4])
    opt = ids == 0
    for T in range(1, 6 * S + 3):
        sd, pd, score = R.viterbi_states(_rand_L(g, 5 * S, T), ids, S, opt)
        assert (sd is None) == (T < 4 * S), T
        if sd is not None:
            assert int(sd.sum()) == T and (sd[~opt] >= 1).all()
            assert all((row == 0).all() or (row >= 1).all() for row in sd)


@pytest.mark.parametrize("S", [1, 2, 3])
def test_t_equal_s_p_gives_one_frame_per_state(S):
    g = np.random.default_rng(10 + S)
    for P in (1, 2, 17):
        ids = g.integers(0, 6, P)
        sd, pd, score = R.viterbi_states(_rand_L(g, 6 * S, S * P), ids, S)
        assert sd.tolist() == [[1] * S] * P and pd.tolist() == [S] * P


@pytest.mark.parametrize("S", [2, 3])
def test_features_at_the_class_means_reproduce_the_generating_state_durations(S):
    V, D = 11, 6
    g = np.random.default_rng(5)
    means = g.normal(0.0, 4.0, (V * S, D))
    model = {"mean": means, "var": np.ones((V * S, D)), "states": S}
    for P in (1, 9, 40):
        ids = g.permutation(V - 1)[np.arange(P) % (V - 1)] + 1               # neighbours (and second neighbours) differ
        sd = g.integers(1, 5, (P, S))
        opt = np.zeros(P, dtype=bool)
        opt[2:P - 2:4] = True
        ids[opt] = 0
        sd[2:P - 2:8] = 0                                                     # every second optional token has no frames
        x = means[R.state_labels(ids, sd, S)]
        got, pd, score = R.viterbi_states(R.loglik(x, model), ids, S, opt)
        assert np.array_equal(got, sd) and np.array_equal(pd, sd.sum(1))
        assert score == pytest.approx(-0.5 * D * math.log(2 * math.pi) * x.shape[0], rel=1e-12)


def test_split_states_and_phone_max():
    assert R.split_states([0, 1, 2, 3, 7], 3).tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [3, 2, 2]]
    assert R.split_states([5], 1).tolist() == [[5]]
    L = np.arange(24.0).reshape(6, 4) * np.array([1, -1, 1, -1])
    assert np.array_equal(R.phone_max(L, 2), np.maximum(L[0::2], L[1::2])) and R.phone_max(L, 2).shape == (3, 4)
    assert np.array_equal(R.phone_max(L, 1), L)


def test_the_hosts_flat_start_is_split_states_and_at_one_state_the_phoneme_per_frame():
    import torch
    from kokoro_ruslan_amd.align import flat_start
    g = torch.Generator().manual_seed(5)
    for S in (1, 2, 3):
        for P in (1, 2, 7, 100):
            ids, d = torch.randint(0, 59, (P,), generator=g), torch.randint(0, 9, (P,), generator=g)
            sd, lab = flat_start(ids, d, S)
            want = R.split_states(d.numpy(), S)
            assert sd.dtype == torch.int64 and np.array_equal(sd.numpy(), want)
            assert np.array_equal(lab.numpy(), R.state_labels(ids.numpy(), want, S))
            if S == 1:
                assert torch.equal(sd, d[:, None]) and torch.equal(lab, torch.repeat_interleave(ids, d))


# The parameters of the comparison below: sub-means N(0, 1) per dimension and noise 1.5 make the two halves of a phone as far from each
# other as from another phone, at a noise level where one Gaussian per phone blurs the boundaries.
PARTS_KW = dict(parts=2, V=12, D=8, mean_std=1.0, noise=1.5)
ACC_1_STATE, ACC_2_STATES = 0.8912, 0.9587                                    # measured with the oracle (fit, fit_states), seed 0


def test_two_states_align_nonstationary_phones_better_than_one():
    """The point of the feature.  On synthetic_corpus_parts(0, parts=2, V=12, D=8, mean_std=1.0, noise=1.5) (40 utterances, every phone
    two stretches with sub-means of their own) the oracle's frame accuracy against the generating phone durations was measured as
        fit        (1 state)   0.8912
        fit_states (2 states)  0.9587
    a gap of 0.0675.  The 2-state accuracy must exceed the 1-state one by half of that gap."""
    feats, ids, _, truth, _, _ = R.synthetic_corpus_parts(0, **PARTS_KW)
    _, d1, _ = R.fit(feats, ids, V=12)
    model, sd2, _ = R.fit_states(feats, ids, V=12, S=2)
    a1 = R.frame_accuracy(ids, d1, truth)
    a2 = R.frame_accuracy(ids, [d.sum(1) for d in sd2], truth)
    print(f"frame accuracy: 1 state {a1:.4f}, 2 states {a2:.4f}, gap {a2 - a1:.4f}")
    assert model["states"] == 2 and model["mean"].shape == (24, 8)
    assert a2 - a1 >= 0.5 * (ACC_2_STATES - ACC_1_STATE)


def test_synthetic_corpus_parts_is_what_it_says():
    feats, ids, opts, durs, means, sdurs = R.synthetic_corpus_parts(3, parts=3, optional=True, n_utts=10)
    assert means.shape == (12, 3, 8)
    skipped = 0
    for x, i, o, d, sd in zip(feats, ids, opts, durs, sdurs):
        assert x.dtype == np.float32 and x.shape == (int(d.sum()), 8) and sd.shape == (len(i), 3)
        assert np.array_equal(sd, R.split_states(d, 3)) and np.array_equal(sd.sum(1), d)
        assert ((d >= 3) | (o & (d == 0))).all() and (i[o] == 0).all() and (i[~o] != 0).all()
        skipped += int((d == 0).sum())
    assert skipped > 0


def test_fit_states_with_optional_tokens_recovers_the_states():
    feats, ids, opts, durs, _, sdurs = R.synthetic_corpus_parts(0, parts=2, optional=True, n_utts=30)
    models = []
    model, sd, scores = R.fit_states(feats, ids, opts, V=12, S=2, models=models)
    assert len(scores) == len(models) <= 6
    acc = R.frame_accuracy(ids, [d.sum(1) for d in sd], durs)
    print(f"frame accuracy {acc:.4f} in {len(scores)} passes")
    assert acc >= 0.97
