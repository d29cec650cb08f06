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
