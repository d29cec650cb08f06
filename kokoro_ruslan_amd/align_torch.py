"""The fp64 oracle of csrc/kk_align.hip: flat-start forced alignment of phoneme tokens to mel frames, on the CPU in numpy.

Written from the definitions (DESIGN §5 "Forced alignment"):
    features    of a log-mel [T, M]: c_1..c_K as dtw_torch.mcep, then c_0 = the frame's mean over the mel channels; from each of these
                K + 1 rows the utterance's own mean over time is subtracted; then the first differences of the normalised rows,
                delta_t = (c_{t+1} - c_{t-1}) / 2 with the edge frames replicated.  D = 2 (K + 1), laid out [T, D] here ([D][T] on the
                device): columns 0..K-1 c_1..c_K, column K c_0, columns K+1..2K+1 their differences in the same order.
    model       per phoneme id v < V a mean mu_v[D] and a variance var_v[D];
                L(v, t) = -1/2 sum_d [(x_d(t) - mu_vd)^2 / var_vd + ln(2 pi var_vd)]
                        = sum over ascending d of a_vd (x_d(t) - mu_vd)^2, plus c_v, with a = -1/2 / var, c = -1/2 sum_d ln(2 pi var).
    alignment   of tokens ids[P] to frames 0..T-1, given optional[P]:
                S(p, t) = L(ids[p], t) + max(S(p, t-1), S(p-1, t-1), S(p-2, t-1) if optional[p-1]);
                codes 0 stay, 1 advance, 2 skip one optional token; a later candidate wins only when strictly greater.
                Start: S(0, 0) = L(ids[0], 0) and, if optional[0], S(1, 0) = L(ids[1], 0).  End: at (P-1, T-1), or at (P-2, T-1) when
                optional[P-1] and that cell is strictly greater.  The only jump is over ONE token, so two adjacent optional tokens
                are never both skipped (a run of optional tokens keeps at least every second one).
    estimation  every frame belongs to the class of its token; per class the count, sum x and sum x^2 give the mean and the (biased)
                variance; a class with fewer than 2 frames takes the global mean and variance; every variance is floored at var_floor
                times the global variance of its dimension (and at VAR_MIN, so that a constant dimension cannot divide by zero).
    fit         Viterbi training from the even split (kokoro.data.features.fallback_durations): estimate -> align, `iters` passes,
                stopping once no duration changes.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from kokoro_ruslan_amd.dtw_torch import _f64, mcep

VAR_MIN = 1e-10
LOG_2PI = math.log(2.0 * math.pi)


def features(mel, K: int = 13) -> np.ndarray:
    """[T, 2 (K + 1)] fp64 of a log-mel [T, M]."""
    x = _f64(mel)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("features needs a log-mel [T >= 1, M]")
    c = mcep(x, K) if K > 0 else np.zeros((x.shape[0], 0))
    s = np.concatenate([c, x.mean(1, keepdims=True)], 1)
    s = s - s.mean(0, keepdims=True)
    e = np.concatenate([s[:1], s, s[-1:]], 0)
    return np.concatenate([s, (e[2:] - e[:-2]) / 2.0], 1)


def loglik_params(model: Dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a [V, D] = -1/2 / var, mu [V, D], c [V] = -1/2 sum_d ln(2 pi var)): what the device stages, in fp64."""
    mu, var = _f64(model["mean"]), _f64(model["var"])
    return -0.5 / var, mu, -0.5 * (LOG_2PI + np.log(var)).sum(1)


def loglik_from_params(feats, a, mu, c) -> np.ndarray:
    """L [V, T] of features [T, D]."""
    x = _f64(feats)
    L = np.empty((a.shape[0], x.shape[0]))
    for v in range(a.shape[0]):
        L[v] = (a[v] * (x - mu[v]) ** 2).sum(1) + c[v]
    return L


def loglik(feats, model: Dict) -> np.ndarray:
    return loglik_from_params(feats, *loglik_params(model))


def viterbi(Lp, optional=None) -> Tuple[Optional[np.ndarray], float]:
    """Lp [P, T]: the score of token p at frame t.  Returns (durations int64 [P] summing to T, score), or (None, -inf) when no path
    exists.  A skipped token gets 0 frames; two adjacent optional tokens are never both skipped."""
    Lp = _f64(Lp)
    P, T = Lp.shape
    if P < 1 or T < 1:
        raise ValueError("viterbi needs at least one token and one frame")
    opt = np.zeros(P, dtype=bool) if optional is None else np.asarray(optional, dtype=bool)
    if opt.shape != (P,):
        raise ValueError(f"{opt.shape[0]} optional flags for {P} tokens")
    ninf = -np.inf
    may_skip = np.concatenate([[False], opt[:-1]])                              # may_skip[p] = optional[p - 1]
    S = np.full(P, ninf)
    S[0] = Lp[0, 0]
    if P > 1 and opt[0]:
        S[1] = Lp[1, 0]
    code = np.zeros((T, P), dtype=np.int8)
    for t in range(1, T):
        best, c = S.copy(), np.zeros(P, dtype=np.int8)
        adv = np.concatenate([[ninf], S[:-1]])
        take = adv > best                                                       # a later candidate only when strictly greater
        best, c = np.where(take, adv, best), np.where(take, np.int8(1), c)
        skip = np.where(may_skip, np.concatenate([[ninf, ninf], S[:-2]])[:P], ninf)
        take = skip > best
        best, c = np.where(take, skip, best), np.where(take, np.int8(2), c)
        S, code[t] = Lp[:, t] + best, c
    p = P - 1
    if P > 1 and opt[P - 1] and S[P - 2] > S[P - 1]:
        p = P - 2
    score = float(S[p])
    if not np.isfinite(score):
        return None, ninf
    dur = np.zeros(P, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        dur[p] += 1
        if t:
            p -= int(code[t, p])
    return dur, score


def align(L, ids, optional=None) -> Tuple[Optional[np.ndarray], float]:
    """viterbi on the rows of L [V, T] the tokens ids[P] name."""
    return viterbi(_f64(L)[np.asarray(ids, dtype=np.int64)], optional)


def path_score(L, ids, durations) -> float:
    """The fp64 score of a given alignment: sum over the frames of L(class of the frame's token, frame)."""
    L, lab = _f64(L), np.repeat(np.asarray(ids, dtype=np.int64), np.asarray(durations, dtype=np.int64))
    return float(L[lab, np.arange(L.shape[1])].sum())


def scores(L, ids, durations) -> Dict:
    """Pronunciation scores of an alignment: L [V, T] finite, ids [P], durations [P] >= 0 summing to T (None: infeasible).  Frame t
    belongs to the token whose span holds it, v(t) is that token's id.  Per frame, in fp64 of the values given: fmax = max_v L(v, t),
    amax = the lowest v that attains it, margin = L(v(t), t) - fmax (<= 0), lpost = margin - log sum_v exp(L(v, t) - fmax) (the log
    posterior under a flat prior), hit = [amax == v(t)].  Per token: frames, gop_sum and lpost_sum (the sums of margin and lpost over
    its frames in ascending order, from 0.0) and hits; a token without frames has zeros.  Per utterance the sums of the tokens' values
    in ascending token order.  Returns {"frames" int64 [P], "gop_sum", "lpost_sum" fp64 [P], "hits" int64 [P], "T", "gop_total",
    "lpost_total", "hits_total", "margin", "lpost" fp64 [T], "amax" int64 [T]}; an infeasible utterance has zeros throughout."""
    L, ids = _f64(L), np.asarray(ids, dtype=np.int64)
    V, T = L.shape
    P = ids.shape[0]
    out = {"frames": np.zeros(P, dtype=np.int64), "gop_sum": np.zeros(P), "lpost_sum": np.zeros(P), "hits": np.zeros(P, dtype=np.int64),
           "T": T, "gop_total": 0.0, "lpost_total": 0.0, "hits_total": 0, "margin": np.zeros(T), "lpost": np.zeros(T),
           "amax": L.argmax(0).astype(np.int64)}                                # (argmax: the first, so the lowest, maximiser)
    if durations is None:
        return out
    d = np.asarray(durations, dtype=np.int64)
    if d.shape != (P,) or (d < 0).any() or int(d.sum()) != T:
        raise ValueError(f"scores needs {P} durations >= 0 that sum to {T}")
    fmax = L.max(0)
    first = 0
    for p in range(P):
        g = l = 0.0
        for t in range(first, first + int(d[p])):
            m = float(L[ids[p], t] - fmax[t])
            lp = m - math.log(float(np.exp(L[:, t] - fmax[t]).sum()))
            out["margin"][t], out["lpost"][t] = m, lp
            g, l = g + m, l + lp
            out["hits"][p] += int(out["amax"][t] == ids[p])
        first += int(d[p])
        out["frames"][p], out["gop_sum"][p], out["lpost_sum"][p] = d[p], g, l
    for p in range(P):
        out["gop_total"] += float(out["gop_sum"][p])
        out["lpost_total"] += float(out["lpost_sum"][p])
        out["hits_total"] += int(out["hits"][p])
    return out


def accumulate(feats: Sequence, labels: Sequence, V: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(count int64 [V], sum x [V, D], sum x^2 [V, D]) over utterances' features [T, D] and frame labels [T] (a label < 0 counts nowhere)."""
    D = _f64(feats[0]).shape[1]
    n, s1, s2 = np.zeros(V, dtype=np.int64), np.zeros((V, D)), np.zeros((V, D))
    for x, lab in zip(feats, labels):
        x, lab = _f64(x), np.asarray(lab, dtype=np.int64)
        for v in np.unique(lab[lab >= 0]):
            sel = x[lab == v]
            n[v] += sel.shape[0]
            s1[v] += sel.sum(0)
            s2[v] += (sel ** 2).sum(0)
    return n, s1, s2


def model_from_stats(n, s1, s2, var_floor: float = 0.01) -> Dict:
    """{"mean", "var"} fp64 [V, D] from the class statistics, by the estimation rule above."""
    n, s1, s2 = np.asarray(n, dtype=np.float64), _f64(s1), _f64(s2)
    N = max(n.sum(), 1.0)
    gmean = s1.sum(0) / N
    gvar = np.maximum(s2.sum(0) / N - gmean ** 2, 0.0)
    safe = np.maximum(n, 1.0)[:, None]
    mean = s1 / safe
    var = s2 / safe - mean ** 2
    few = n < 2
    mean[few], var[few] = gmean, gvar
    return {"mean": mean, "var": np.maximum(np.maximum(var, var_floor * gvar), VAR_MIN)}


def even_split(P: int, T: int) -> np.ndarray:
    """kokoro.data.features.fallback_durations: T frames spread evenly over P tokens, the remainder one each to the first ones."""
    d = np.full(P, T // P, dtype=np.int64)
    d[:T % P] += 1
    return d


def fit(feats: Sequence, ids: Sequence, optional: Optional[Sequence] = None, V: int = 59, iters: int = 6, var_floor: float = 0.01,
        models: Optional[List] = None):
    """Viterbi training on features [T, D] per utterance.  Returns (model, durations: list of int64 [P] | None, scores: the corpus
    score of each pass's alignment).  An infeasible utterance has durations None and takes no part in the next estimate.  models: a
    list that receives the model of every pass."""
    ids = [np.asarray(i, dtype=np.int64) for i in ids]
    optional = [None] * len(ids) if optional is None else list(optional)
    durs: List[Optional[np.ndarray]] = [even_split(len(i), _f64(x).shape[0]) for x, i in zip(feats, ids)]
    model, scores = None, []
    for _ in range(iters):
        labels = [np.repeat(i, d) if d is not None else np.full(_f64(x).shape[0], -1) for x, i, d in zip(feats, ids, durs)]
        model = model_from_stats(*accumulate(feats, labels, V), var_floor=var_floor)
        if models is not None:
            models.append(model)
        a, mu, c = loglik_params(model)
        new, total = [], 0.0
        for x, i, o in zip(feats, ids, optional):
            d, s = align(loglik_from_params(x, a, mu, c), i, o)
            new.append(d)
            total += s if d is not None else 0.0
        scores.append(total)
        same = all((d is None and e is None) or (d is not None and e is not None and np.array_equal(d, e)) for d, e in zip(durs, new))
        durs = new
        if same:
            break
    return model, durs, scores


def synthetic_corpus(seed: int, optional: bool = False, n_utts: int = 40, V: int = 12, D: int = 8, mean_std: float = 2.0,
                     noise: float = 0.5):
    """A corpus with a known alignment: class means N(0, mean_std^2) per dimension, frames = the class mean + N(0, noise^2); 5-20
    tokens per utterance of 1-12 frames each.  With `optional`, a quarter of the inner tokens are optional tokens of class 0 (which
    no other token uses), half of them zero-length, no two of them adjacent.  Returns (feats: list of fp32 [T, D], ids: list of int64
    [P], optional: list of bool [P], durations: list of int64 [P], means [V, D])."""
    g = np.random.default_rng(seed)
    means = g.normal(0.0, mean_std, (V, D))
    feats, ids, opts, durs = [], [], [], []
    for _ in range(n_utts):
        P = int(g.integers(5, 21))
        i = g.integers(1 if optional else 0, V, P)
        o = np.zeros(P, dtype=bool)
        d = g.integers(1, 13, P)
        if optional:
            for p in range(1, P - 1):
                if not o[p - 1] and g.random() < 0.25:
                    o[p], i[p] = True, 0
                    if g.random() < 0.5:
                        d[p] = 0
        lab = np.repeat(i, d)
        feats.append((means[lab] + g.normal(0.0, noise, (lab.shape[0], D))).astype(np.float32))
        ids.append(i.astype(np.int64)), opts.append(o), durs.append(d.astype(np.int64))
    return feats, ids, opts, durs, means


def frame_accuracy(ids: Sequence, durations: Sequence, truth: Sequence) -> float:
    """The share of frames whose class under `durations` is their class under `truth`."""
    good = total = 0
    for i, d, t in zip(ids, durations, truth):
        want = np.repeat(i, t)
        total += want.shape[0]
        if d is not None:
            good += int((np.repeat(i, d) == want).sum())
    return good / max(total, 1)


# ---- multi-state phone models: a left-to-right chain of S states per phoneme (DESIGN §5 "Forced alignment", "States") -----------------
# The classes are c = v S + j, j = 0..S-1; a model is {"mean", "var"} [V S, D] plus "states": S, and L is [V S, T].  loglik_params,
# loglik_from_params, accumulate and model_from_stats above take V S as their class count.

def viterbi_states(L, ids, S: int, optional=None):
    """L [V S, T], ids [P].  State (p, j) of token p scores
        Sigma(p, j, t) = L(ids[p] S + j, t) + max of, in this order, a later candidate only when strictly greater:
            code 0 stay     Sigma(p, j, t-1)
            code 1 advance  Sigma(p, j-1, t-1) if j > 0, else Sigma(p-1, S-1, t-1)
            code 2 skip     Sigma(p-2, S-1, t-1), only for j = 0 and optional[p-1].
    Start: (0, 0) and, if optional[0], (1, 0).  End: (P-1, S-1), or (P-2, S-1) when optional[P-1] and that cell is strictly greater.
    A skipped token loses all its states; a present one has >= 1 frame in each.  Returns (state durations int64 [P, S], phone durations
    int64 [P] = their row sums, score), or (None, None, -inf) when no path exists.  With S = 1 this is `viterbi`, operation by operation."""
    L, ids = _f64(L), np.asarray(ids, dtype=np.int64)
    if int(S) != S or S < 1:
        raise ValueError(f"states must be an integer >= 1, not {S!r}")
    S = int(S)
    P, T = ids.shape[0], L.shape[1]
    if P < 1 or T < 1:
        raise ValueError("viterbi_states needs at least one token and one frame")
    if L.shape[0] % S or (ids < 0).any() or (ids >= L.shape[0] // S).any():
        raise ValueError(f"L has {L.shape[0]} classes: not {S} states each of the ids given")
    opt = np.zeros(P, dtype=bool) if optional is None else np.asarray(optional, dtype=bool)
    if opt.shape != (P,):
        raise ValueError(f"{opt.shape[0]} optional flags for {P} tokens")
    ninf = -np.inf
    Lp = L[ids[:, None] * S + np.arange(S)[None, :]]                            # [P, S, T]
    may_skip = np.concatenate([[False], opt[:-1]])
    sig = np.full((P, S), ninf)
    sig[0, 0] = Lp[0, 0, 0]
    if P > 1 and opt[0]:
        sig[1, 0] = Lp[1, 0, 0]
    code = np.zeros((T, P, S), dtype=np.int8)
    for t in range(1, T):
        best, c = sig.copy(), np.zeros((P, S), dtype=np.int8)
        adv = np.empty((P, S))
        adv[:, 1:], adv[0, 0], adv[1:, 0] = sig[:, :-1], ninf, sig[:-1, S - 1]
        take = adv > best
        best, c = np.where(take, adv, best), np.where(take, np.int8(1), c)
        skip = np.full((P, S), ninf)
        skip[:, 0] = np.where(may_skip, np.concatenate([[ninf, ninf], sig[:-2, S - 1]])[:P], ninf)
        take = skip > best
        best, c = np.where(take, skip, best), np.where(take, np.int8(2), c)
        sig, code[t] = Lp[:, :, t] + best, c
    p, j = P - 1, S - 1
    if P > 1 and opt[P - 1] and sig[P - 2, j] > sig[P - 1, j]:
        p = P - 2
    score = float(sig[p, j])
    if not np.isfinite(score):
        return None, None, ninf
    sd = np.zeros((P, S), dtype=np.int64)
    for t in range(T - 1, -1, -1):
        sd[p, j] += 1
        if t:
            c = int(code[t, p, j])
            if c == 1 and j > 0:
                j -= 1
            elif c:
                p, j = p - c, S - 1
    return sd, sd.sum(1), score


def state_labels(ids, state_durations, S: int) -> np.ndarray:
    """The class ids[p] S + j of every frame under state durations [P, S]."""
    cls = np.asarray(ids, dtype=np.int64)[:, None] * int(S) + np.arange(int(S))[None, :]
    return np.repeat(cls.ravel(), np.asarray(state_durations, dtype=np.int64).reshape(-1))


def path_score_states(L, ids, state_durations, S: int) -> float:
    """The fp64 score of a given state alignment: sum over the frames of L(class of the frame's state, frame)."""
    L, lab = _f64(L), state_labels(ids, state_durations, S)
    return float(L[lab, np.arange(L.shape[1])].sum())


def split_states(durations, S: int) -> np.ndarray:
    """[P, S]: each token's d frames spread over its S states as even_split(S, d) spreads them (a state may get none)."""
    d = np.asarray(durations, dtype=np.int64).reshape(-1)
    return np.stack([even_split(int(S), int(x)) for x in d]) if d.shape[0] else np.zeros((0, int(S)), dtype=np.int64)


def phone_max(L, S: int) -> np.ndarray:
    """[V S, T] -> [V, T]: a frame's phone likelihood is that of the phone's best state (exact: a maximum does not round)."""
    L = _f64(L)
    return L.reshape(L.shape[0] // int(S), int(S), L.shape[1]).max(1)


def fit_states(feats: Sequence, ids: Sequence, optional: Optional[Sequence] = None, V: int = 59, S: int = 2, iters: int = 6,
               var_floor: float = 0.01, models: Optional[List] = None):
    """`fit` with S states per phoneme.  Pass 0's labels come from even_split(P, T) per utterance, then split_states; then estimate ->
    viterbi_states, stopping once no state duration changes.  Returns (model with "states", state durations: list of int64 [P, S] |
    None, scores).  The phone durations are the row sums."""
    ids = [np.asarray(i, dtype=np.int64) for i in ids]
    optional = [None] * len(ids) if optional is None else list(optional)
    durs: List[Optional[np.ndarray]] = [split_states(even_split(len(i), _f64(x).shape[0]), S) for x, i in zip(feats, ids)]
    model, scores = None, []
    for _ in range(iters):
        labels = [state_labels(i, d, S) if d is not None else np.full(_f64(x).shape[0], -1) for x, i, d in zip(feats, ids, durs)]
        model = dict(model_from_stats(*accumulate(feats, labels, V * S), var_floor=var_floor), states=int(S))
        if models is not None:
            models.append(model)
        a, mu, c = loglik_params(model)
        new, total = [], 0.0
        for x, i, o in zip(feats, ids, optional):
            d, _, s = viterbi_states(loglik_from_params(x, a, mu, c), i, S, o)
            new.append(d)
            total += s if d is not None else 0.0
        scores.append(total)
        same = all((d is None and e is None) or (d is not None and e is not None and np.array_equal(d, e)) for d, e in zip(durs, new))
        durs = new
        if same:
            break
    return model, durs, scores


def synthetic_corpus_parts(seed: int, parts: int = 2, optional: bool = False, n_utts: int = 40, V: int = 12, D: int = 8,
                           mean_std: float = 2.0, noise: float = 0.5, max_frames: int = 12):
    """synthetic_corpus with phones that are not stationary: every class has `parts` sub-means drawn independently, N(0, mean_std^2)
    per dimension, and a token of d frames is split_states(d, parts) stretches of them in order (every present token has parts..
    max_frames frames, so each stretch has at least one).  Returns (feats, ids, optional, durations, means [V, parts, D], state
    durations: list of int64 [P, parts])."""
    g = np.random.default_rng(seed)
    means = g.normal(0.0, mean_std, (V, parts, D))
    feats, ids, opts, durs, sdurs = [], [], [], [], []
    for _ in range(n_utts):
        P = int(g.integers(5, 21))
        i = g.integers(1 if optional else 0, V, P)
        o = np.zeros(P, dtype=bool)
        d = g.integers(parts, max_frames + 1, P)
        if optional:
            for p in range(1, P - 1):
                if not o[p - 1] and g.random() < 0.25:
                    o[p], i[p] = True, 0
                    if g.random() < 0.5:
                        d[p] = 0
        sd = split_states(d, parts)
        lab = state_labels(i, sd, parts)
        feats.append((means.reshape(V * parts, D)[lab] + g.normal(0.0, noise, (lab.shape[0], D))).astype(np.float32))
        ids.append(i.astype(np.int64)), opts.append(o), durs.append(d.astype(np.int64)), sdurs.append(sd)
    return feats, ids, opts, durs, means, sdurs


# ---- Gaussian mixtures per state: M = 2 or 4 diagonal components per class (DESIGN §5 "Forced alignment", "Mixtures") -----------------
# C = V S classes as above, G = C M Gaussians: Gaussian c M + m is component m of class c.  A model is {"mean", "var"} [G, D],
# "weight" [C, M] (rows summing to 1) and "mixtures": M, plus "states" as above; a model without "mixtures" is M = 1.
#     l_m(t) = sum over ascending d of a[g][d] (x_d - mu[g][d])^2, plus k[g], k[g] = ln w_cm - 1/2 sum_d ln(2 pi var)
#     L(c, t) = mx + log sum over ascending m of exp(l_m - mx), mx = max_m l_m
# Training assigns every frame to ONE component of its class (the largest l_m, the lowest m on a tie), as Viterbi training assigns
# it to one class.

SPLIT = 0.2                                                                     # a split moves the two children by -/+ SPLIT sqrt(var)


def mixtures_of(model: Dict) -> int:
    return int(model.get("mixtures", 1))


def loglik_mix_params(model: Dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a [G, D], mu [G, D], k [G] = ln w - 1/2 sum_d ln(2 pi var)) in fp64; without "weight" (M = 1) k is loglik_params' c."""
    a, mu, c = loglik_params(model)
    if "weight" not in model:
        return a, mu, c
    with np.errstate(divide="ignore"):
        return a, mu, np.log(_f64(model["weight"])).reshape(-1) + c


def mix_components(feats, a, mu, k) -> np.ndarray:
    """l [G, T]: every component's value, weight included."""
    return loglik_from_params(feats, a, mu, k)


def loglik_mix_from_params(feats, a, mu, k, M: int) -> np.ndarray:
    """L [C, T] of features [T, D] from the G = C M components' parameters.  A class needs one finite component at least."""
    l = mix_components(feats, a, mu, k)
    if int(M) == 1:
        return l
    l = l.reshape(l.shape[0] // int(M), int(M), l.shape[1])
    mx = l.max(1)
    s = np.zeros_like(mx)
    for m in range(int(M)):                                                     # ascending m
        s = s + np.exp(l[:, m] - mx)
    return mx + np.log(s)


def loglik_mix(feats, model: Dict) -> np.ndarray:
    return loglik_mix_from_params(feats, *loglik_mix_params(model), mixtures_of(model))


def mix_labels_from_params(feats, labels, a, mu, k, M: int) -> np.ndarray:
    """[T]: label M + the component of the frame's class `label` with the largest value (the lowest on a tie); -1 where label < 0."""
    M, lab = int(M), np.asarray(labels, dtype=np.int64)
    l = mix_components(feats, a, mu, k)
    l = l.reshape(l.shape[0] // M, M, l.shape[1])
    t = np.arange(lab.shape[0])
    best = l[np.maximum(lab, 0), :, t].argmax(1)                                # (argmax: the first, so the lowest, maximiser)
    return np.where(lab >= 0, lab * M + best, -1)


def split_mixtures(model: Dict) -> Dict:
    """M -> 2 M: component m of a class becomes 2 m at mu - SPLIT sqrt(var) and 2 m + 1 at mu + SPLIT sqrt(var), each with the
    variance copied and half the weight.  A model without "weight" is M = 1 with weight 1."""
    mu, var = _f64(model["mean"]), _f64(model["var"])
    M = mixtures_of(model)
    w = _f64(model["weight"]) if "weight" in model else np.ones((mu.shape[0], 1))
    step = SPLIT * np.sqrt(var)
    out = {k: v for k, v in model.items() if k not in ("mean", "var", "weight", "mixtures")}
    out.update(mean=np.stack([mu - step, mu + step], 1).reshape(2 * mu.shape[0], -1), var=np.repeat(var, 2, 0),
               weight=np.repeat(w / 2.0, 2, 1), mixtures=2 * M)
    return out


def model_from_mix_stats(n, s1, s2, M: int, var_floor: float = 0.01) -> Dict:
    """{"mean", "var" [G, D], "weight" [C, M], "mixtures"} from the Gaussians' statistics n [G], s1, s2 [G, D].
    weight: w_cm = (n_cm + 1) / (n_c + M), strictly positive.  A class's pooled mean and variance come from the sums over its
    components, or, with n_c < 2, from the global ones.  A component with n_cm < 2 is seeded again from its class's pooled statistics
    where its index stood at the split that made it: the pooled mean - SPLIT sqrt(pooled var) for an even m, + for an odd one, with the
    pooled variance.  Every variance is floored at var_floor times the global variance and at VAR_MIN."""
    M = int(M)
    n, s1, s2 = np.asarray(n, dtype=np.float64), _f64(s1), _f64(s2)
    G, D = s1.shape
    C = G // M
    N = max(n.sum(), 1.0)
    gmean = s1.sum(0) / N
    gvar = np.maximum(s2.sum(0) / N - gmean ** 2, 0.0)
    nc = n.reshape(C, M).sum(1)
    safe = np.maximum(nc, 1.0)[:, None]
    cmean = s1.reshape(C, M, D).sum(1) / safe
    cvar = np.maximum(s2.reshape(C, M, D).sum(1) / safe - cmean ** 2, 0.0)
    cmean[nc < 2], cvar[nc < 2] = gmean, gvar
    safe = np.maximum(n, 1.0)[:, None]
    mean = s1 / safe
    var = s2 / safe - mean ** 2
    sign = np.where(np.arange(G) % 2 == 0, -1.0, 1.0)[:, None]
    few = n < 2
    mean[few] = (np.repeat(cmean, M, 0) + sign * SPLIT * np.sqrt(np.repeat(cvar, M, 0)))[few]
    var[few] = np.repeat(cvar, M, 0)[few]
    return {"mean": mean, "var": np.maximum(np.maximum(var, var_floor * gvar), VAR_MIN),
            "weight": (n.reshape(C, M) + 1.0) / (nc[:, None] + M), "mixtures": M}


def fit_mix(feats: Sequence, ids: Sequence, optional: Optional[Sequence] = None, V: int = 59, S: int = 1, M: int = 2, iters: int = 6,
            mix_iters: int = 4, var_floor: float = 0.01, models: Optional[List] = None):
    """fit_states (the single-Gaussian training, all of it), then mixing up: for each doubling 1 -> 2 (-> 4) split_mixtures, then up
    to mix_iters passes of
        align with the current model (loglik_mix -> viterbi_states), assign components (mix_labels), accumulate, estimate,
    a doubling's passes ending early once no state duration and no count changes; at the end one closing alignment with the last
    estimate, so that the durations returned are the model's own.  Returns (model, state durations: list of int64 [P, S] | None,
    scores: fit_states' and then one per mixture alignment, the closing one included).  models: receives the model every mixture
    alignment used."""
    if M not in (1, 2, 4):
        raise ValueError(f"mixtures must be 1, 2 or 4, not {M!r}")
    ids = [np.asarray(i, dtype=np.int64) for i in ids]
    optional = [None] * len(ids) if optional is None else list(optional)
    model, durs, scores = fit_states(feats, ids, optional, V=V, S=S, iters=iters, var_floor=var_floor)
    if M == 1:
        return model, durs, scores
    C = V * int(S)

    def align_all(model):
        a, mu, k = loglik_mix_params(model)
        new, total = [], 0.0
        for x, i, o in zip(feats, ids, optional):
            d, _, s = viterbi_states(loglik_mix_from_params(x, a, mu, k, model["mixtures"]), i, S, o)
            new.append(d)
            total += s if d is not None else 0.0
        if models is not None:
            models.append(model)
        scores.append(total)
        return new, (a, mu, k)

    while mixtures_of(model) < M:
        model = dict(split_mixtures(model), states=int(S))
        m, counts = model["mixtures"], None
        for _ in range(mix_iters):
            new, prm = align_all(model)
            labels = [mix_labels_from_params(x, state_labels(i, d, S), *prm, m) if d is not None else np.full(_f64(x).shape[0], -1)
                      for x, i, d in zip(feats, ids, new)]
            n, s1, s2 = accumulate(feats, labels, C * m)
            model = dict(model_from_mix_stats(n, s1, s2, m, var_floor=var_floor), states=int(S))
            same = counts is not None and np.array_equal(n, counts) and all(
                (d is None and e is None) or (d is not None and e is not None and np.array_equal(d, e)) for d, e in zip(durs, new))
            durs, counts = new, n
            if same:
                break
    durs, _ = align_all(model)
    return model, durs, scores


def synthetic_corpus_modes(seed: int, modes: int = 2, optional: bool = False, n_utts: int = 40, V: int = 12, D: int = 8,
                           mean_std: float = 2.0, noise: float = 1.0, max_frames: int = 12):
    """synthetic_corpus with phones that have allophones: every class has `modes` means drawn independently, N(0, mean_std^2) per
    dimension (well separated against `noise`), every token draws one of its class's modes and emits all its frames around that mean.
    One Gaussian over such a class has the spread of its modes as its variance.  Returns (feats, ids, optional, durations, means [V,
    modes, D], modes: list of int64 [P], the mode of every token)."""
    g = np.random.default_rng(seed)
    means = g.normal(0.0, mean_std, (V, modes, D))
    feats, ids, opts, durs, picks = [], [], [], [], []
    for _ in range(n_utts):
        P = int(g.integers(5, 21))
        i = g.integers(1 if optional else 0, V, P)
        o = np.zeros(P, dtype=bool)
        d = g.integers(1, max_frames + 1, P)
        k = g.integers(0, modes, P)
        if optional:
            for p in range(1, P - 1):
                if not o[p - 1] and g.random() < 0.25:
                    o[p], i[p] = True, 0
                    if g.random() < 0.5:
                        d[p] = 0
        lab = np.repeat(i * modes + k, d)
        feats.append((means.reshape(V * modes, D)[lab] + g.normal(0.0, noise, (lab.shape[0], D))).astype(np.float32))
        ids.append(i.astype(np.int64)), opts.append(o), durs.append(d.astype(np.int64)), picks.append(k.astype(np.int64))
    return feats, ids, opts, durs, means, picks
