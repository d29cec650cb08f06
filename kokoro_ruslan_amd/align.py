"""Flat-start forced alignment on the device, on the kernels of csrc/kk_align.hip: phoneme durations without an external aligner.

What a monophone first stage does, reduced to essentials: one diagonal Gaussian per phoneme id over cepstral features of the log-mel
(c_1..c_K and c_0, mean-normalised per utterance, plus their first differences), a flat start from the even split, and a few passes of
Viterbi training: align every utterance with the current Gaussians, re-estimate the Gaussians from the alignment.  `PhoneAligner.fit`
does that over a corpus held as lists, `align` aligns with a given model; an utterance's result is, bit for bit, what it gives alone.
`score` aligns and says how well the frames fit the phonemes they were aligned to (goodness of pronunciation, log posterior, frame
accuracy, per token and per utterance).  align_torch is the fp64 oracle of every step.

`PhoneAligner(states=S)`, S = 2 or 3, gives every phoneme a left-to-right chain of S states, each with its own Gaussian (class v S + j):
a token that has frames has at least S, one per state.  Everything follows the aligner's `states`; 1 is the default and changes nothing.

`PhoneAligner(mixtures=M)`, M = 2 or 4, gives every class (state) a mixture of M diagonal Gaussians, Gaussian c M + m component m of
class c, with weights [C, M]: L(c, t) is the log of the weighted sum of its components (kk_align_loglik).  `fit` trains the single
Gaussians as always, then mixes up: split every component in two, a few passes that assign every frame to the best component of its
class, double again.  Alignment and scores see only L [C, T]; 1 is the default and changes nothing.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.align_torch import SPLIT, VAR_MIN, even_split
from kokoro_ruslan_amd.dtw_torch import dct_table

MAX_FRAMES = 4096                        # the longest utterance the kernels take (the positional table's order)
MAX_MEL = 128                            # kk_mcep stages 64 frames of at most this many channels
MAX_CLASSES = 256                        # kk_align_loglik
MAX_DIM = 64
MAX_STATES = 3                           # kk_align_viterbi
MIXTURES = (1, 2, 4)                     # components per class: kk_align_loglik
MAX_GAUSSIANS = 1024                     # classes x components


def max_tokens() -> int:
    """Tokens of an utterance the Viterbi kernel takes: the size of its workgroup."""
    return int(kk.load().kk_align_max_tokens())


def mix_frames() -> int:
    """Frames per workgroup of the mixture kernels."""
    return int(kk.load().kk_align_mix_frames())


def code_words(P: int, T: int, S: int = 1) -> int:
    """32-bit code words of a P-token, T-frame utterance with S states per token: 16 tokens of a (frame, state) per word, [T][S][W]."""
    return T * S * ((P + 15) // 16)


def flat_start(ids: torch.Tensor, d: torch.Tensor, S: int):
    """The labels Viterbi training starts from: tokens ids [P] with d [P] frames each, every token's frames spread over its S states as
    align_torch.split_states spreads them.  (state durations [P, S], the class ids[p] S + j of every frame); with S = 1 these are d[:, None]
    and repeat_interleave(ids, d)."""
    j = torch.arange(S)[None, :]
    sd = torch.div(d[:, None], S, rounding_mode="floor") + (j < (d % S)[:, None])
    return sd, torch.repeat_interleave((ids[:, None] * S + j).reshape(-1), sd.reshape(-1))


class PhoneAligner:
    """Batched Viterbi alignment and Viterbi training on the MI355X."""

    def __init__(self, device: str = "cuda", K: int = 13, n_classes: int = 59, var_floor: float = 0.01, states: int = 1,
                 mixtures: int = 1):
        if int(K) != K or not (0 <= K <= MAX_DIM // 2 - 1):
            raise ValueError(f"K must be an integer in 0..{MAX_DIM // 2 - 1}, not {K!r}")
        if int(n_classes) != n_classes or not (1 <= n_classes <= MAX_CLASSES):
            raise ValueError(f"n_classes must be an integer in 1..{MAX_CLASSES}, not {n_classes!r}")
        if not (0.0 <= var_floor < 1.0):
            raise ValueError(f"var_floor must be in [0, 1), not {var_floor!r}")
        if int(states) != states or not (1 <= states <= MAX_STATES):
            raise ValueError(f"states must be an integer in 1..{MAX_STATES}, not {states!r}")
        if mixtures not in MIXTURES:
            raise ValueError(f"mixtures must be 1, 2 or 4, not {mixtures!r}")
        if n_classes * states * mixtures > MAX_GAUSSIANS:
            raise ValueError(f"{n_classes} phoneme ids of {states} states and {mixtures} components are {n_classes * states * mixtures} "
                             f"Gaussians; at most {MAX_GAUSSIANS}")
        if n_classes * states > MAX_CLASSES:
            raise ValueError(f"{n_classes} phoneme ids of {states} states are {n_classes * states} classes; at most {MAX_CLASSES}")
        self.device, self.K, self.n_classes, self.var_floor = torch.device(device), int(K), int(n_classes), float(var_floor)
        self.states, self.mixtures = int(states), int(mixtures)
        self.state_durations: Optional[List[Optional[torch.Tensor]]] = None      # of the last fit(), when states > 1
        self._tables: Dict[int, torch.Tensor] = {}

    @property
    def dim(self) -> int:
        return 2 * (self.K + 1)

    @property
    def classes(self) -> int:
        """Classes of the model: `states` per phoneme id, class v states + j."""
        return self.n_classes * self.states

    @property
    def gaussians(self) -> int:
        """Gaussians of the model: `mixtures` per class, Gaussian c mixtures + m."""
        return self.classes * self.mixtures

    # ---- guards: everything is checked before anything is launched --------------------------------------------------------------
    def _check(self, mels, ids, feats) -> None:
        x, what = (mels, "mel") if feats is None else (feats, "features")
        if x is None or len(x) != len(ids):
            raise ValueError(f"{0 if x is None else len(x)} {what} tensors for {len(ids)} token sequences")
        if not len(ids):
            raise ValueError("nothing to align")
        limit = max_tokens()
        for i, (m, t) in enumerate(zip(x, ids)):
            if not isinstance(m, torch.Tensor) or m.dim() != 2 or not m.is_floating_point():
                raise ValueError(f"utterance {i}: the {what} must be a float tensor [frames, {'mels' if feats is None else 'dims'}]")
            if m.shape[0] < 1:
                raise ValueError(f"utterance {i}: the {what} is empty")
            if m.shape[0] > MAX_FRAMES:
                raise ValueError(f"utterance {i}: {m.shape[0]} frames; at most {MAX_FRAMES}")
            if feats is None and m.shape[1] > MAX_MEL:
                raise ValueError(f"utterance {i}: {m.shape[1]} mel channels; at most {MAX_MEL}")
            if m.shape[1] != x[0].shape[1] or m.shape[1] < 1:
                raise ValueError(f"utterance {i}: {m.shape[1]} channels against {x[0].shape[1]}")
            if feats is not None and m.shape[1] > MAX_DIM:
                raise ValueError(f"utterance {i}: {m.shape[1]} feature dimensions; at most {MAX_DIM}")
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.is_floating_point():
                raise ValueError(f"utterance {i}: the tokens must be an integer tensor [P]")
            if t.shape[0] < 1:
                raise ValueError(f"utterance {i}: no tokens")
            if t.shape[0] > limit:
                raise ValueError(f"utterance {i}: {t.shape[0]} tokens; at most {limit}")
            if int(t.min()) < 0 or int(t.max()) >= self.n_classes:
                raise ValueError(f"utterance {i}: phoneme ids must lie in 0..{self.n_classes - 1}")

    def _check_tags(self, model: Dict) -> None:
        for k, mine in (("states", self.states), ("mixtures", self.mixtures)):
            if int(model.get(k, 1)) != mine:
                raise ValueError(f"the model has {k} = {int(model.get(k, 1))}; this aligner has {k} = {mine}")

    def _check_model(self, model: Dict, D: int) -> None:
        self._check_tags(model)
        for k in ("mean", "var"):
            if tuple(model[k].shape) != (self.gaussians, D):
                raise ValueError(f"the model's {k} is {tuple(model[k].shape)}; this aligner and these features need ({self.gaussians}, {D})")
        if self.mixtures > 1 and tuple(model["weight"].shape) != (self.classes, self.mixtures):
            raise ValueError(f"the model's weight is {tuple(model['weight'].shape)}; this aligner needs ({self.classes}, {self.mixtures})")

    # ---- pieces ------------------------------------------------------------------------------------------------------------------
    def table(self, M: int) -> torch.Tensor:
        if M not in self._tables:
            self._tables[M] = torch.from_numpy(dct_table(M, self.K)).to(torch.float32).to(self.device).contiguous()
        return self._tables[M]

    def _features_packed(self, x: torch.Tensor, foff: torch.Tensor, B: int) -> torch.Tensor:
        T, M = x.shape
        cep = None
        if self.K:
            cep = torch.empty(self.K, T, dtype=torch.float32, device=self.device)
            kk.call("kk_mcep", x, T, M, self.K, self.table(M), cep)
        feat = torch.empty(self.dim, T, dtype=torch.float32, device=self.device)
        kk.call("kk_align_feats", cep, x, T, M, self.K, foff, B, feat)
        return feat

    def features(self, mels: Sequence[torch.Tensor]) -> torch.Tensor:
        """The packed features [D, T_total] (fp32, on the device) of log-mels [T, M]: utterance after utterance along time."""
        self._check(mels, [torch.zeros(1, dtype=torch.long)] * len(mels), None)
        x = torch.cat([m.to(self.device, torch.float32) for m in mels]).contiguous()
        foff = kk.packed_offsets([int(m.shape[0]) for m in mels], torch.int32, self.device)
        return self._features_packed(x, foff, len(mels))

    def params(self, model: Dict):
        """(a = -1/2 / var, mu, c = -1/2 sum ln(2 pi var)) as the device takes them: evaluated in fp64, rounded once.  A mixture model
        has these per Gaussian [G], and c is k = ln w + c (a weight of 0 gives -inf: the component is dropped)."""
        mean, var = model["mean"].to(torch.float64), model["var"].to(torch.float64)
        a, c = -0.5 / var, -0.5 * (math.log(2.0 * math.pi) + var.log()).sum(1)
        if "weight" in model:
            c = model["weight"].to(c.device, torch.float64).log().reshape(-1) + c
        return tuple(t.to(torch.float32).to(self.device).contiguous() for t in (a, mean, c))

    def loglik(self, feat: torch.Tensor, model: Dict) -> torch.Tensor:
        """L [V, T_total] (fp32) of packed features [D, T_total] on the device."""
        D, T = feat.shape
        self._check_model(model, D)
        a, mu, c = self.params(model)
        L = torch.empty(self.classes, T, dtype=torch.float32, device=self.device)
        kk.call("kk_align_loglik", feat, T, D, self.classes, self.mixtures, a, mu, c, L)
        return L

    def mix_labels(self, feat: torch.Tensor, model: Dict, label: torch.Tensor) -> torch.Tensor:
        """int32 [T_total]: label[t] M + the best component of class label[t] at frame t (the lowest on a tie), -1 where label is."""
        D, T = feat.shape
        self._check_model(model, D)
        a, mu, k = self.params(model)
        out = torch.empty(T, dtype=torch.int32, device=self.device)
        kk.call("kk_align_mix_labels", feat, T, D, self.classes, self.mixtures, a, mu, k, label, out)
        return out

    def accumulate_mix(self, feat: torch.Tensor, mixlabel: torch.Tensor, G: Optional[int] = None):
        """accumulate() over G Gaussians (default: this aligner's) by a counting sort of the frames: (count [G], sum x, sum x^2 [G, D])."""
        D, T = feat.shape
        G = self.gaussians if G is None else int(G)
        count = torch.empty(G, dtype=torch.int64, device=self.device)
        sums = torch.empty(2, G, D, dtype=torch.float64, device=self.device)
        ws = torch.empty(max(int(kk.load().kk_align_accumulate_mix_ws_bytes(T, G)), 4), dtype=torch.uint8, device=self.device)
        kk.call("kk_align_accumulate_mix", feat, mixlabel, T, D, G, count, sums[0], sums[1], ws, ws.numel())
        return count, sums[0], sums[1]

    def accumulate(self, feat: torch.Tensor, label: torch.Tensor):
        """(count int64 [V], sum x fp64 [V, D], sum x^2 fp64 [V, D]) of packed features [D, T_total] under frame labels int32 [T_total]."""
        D, T = feat.shape
        V = self.classes
        count = torch.empty(V, dtype=torch.int64, device=self.device)
        sums = torch.empty(2, V, D, dtype=torch.float64, device=self.device)
        kk.call("kk_align_accumulate", feat, label, T, D, V, count, sums[0], sums[1])
        return count, sums[0], sums[1]

    def estimate(self, count: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor) -> Dict:
        """The model of class statistics (align_torch.model_from_stats, in fp64 torch): [V, D] is tiny."""
        n = count.to(torch.float64)
        N = n.sum().clamp(min=1.0)
        gmean = s1.sum(0) / N
        gvar = (s2.sum(0) / N - gmean ** 2).clamp(min=0.0)
        safe = n.clamp(min=1.0)[:, None]
        mean = s1 / safe
        var = s2 / safe - mean ** 2
        few = (n < 2)[:, None]
        mean, var = torch.where(few, gmean, mean), torch.where(few, gvar, var)
        var = torch.maximum(torch.maximum(var, self.var_floor * gvar), torch.full_like(var, VAR_MIN))
        return self._model(mean, var)

    def split(self, model: Dict) -> Dict:
        """M -> 2 M (align_torch.split_mixtures): component m becomes 2 m at mu - SPLIT sqrt(var) and 2 m + 1 at mu + SPLIT sqrt(var),
        the variance copied, the weight halved.  The aligner's `mixtures` is not consulted: fit() walks 1 -> 2 -> 4 with it."""
        mu, var = model["mean"].to(torch.float64), model["var"].to(torch.float64)
        w = model["weight"].to(mu.device, torch.float64) if "weight" in model else torch.ones(mu.shape[0], 1, dtype=torch.float64, device=mu.device)
        step = SPLIT * var.sqrt()
        return self._model(torch.stack([mu - step, mu + step], 1).reshape(2 * mu.shape[0], -1), var.repeat_interleave(2, 0),
                           (w / 2.0).repeat_interleave(2, 1), 2 * int(model.get("mixtures", 1)))

    def estimate_mix(self, count: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, M: int) -> Dict:
        """The mixture model of the Gaussians' statistics (align_torch.model_from_mix_stats, in fp64 torch)."""
        G, D = s1.shape
        C = G // M
        n = count.to(torch.float64)
        N = n.sum().clamp(min=1.0)
        gmean = s1.sum(0) / N
        gvar = (s2.sum(0) / N - gmean ** 2).clamp(min=0.0)
        nc = n.view(C, M).sum(1)
        safe = nc.clamp(min=1.0)[:, None]
        cmean = s1.view(C, M, D).sum(1) / safe
        cvar = (s2.view(C, M, D).sum(1) / safe - cmean ** 2).clamp(min=0.0)
        lone = (nc < 2)[:, None]
        cmean, cvar = torch.where(lone, gmean, cmean).repeat_interleave(M, 0), torch.where(lone, gvar, cvar).repeat_interleave(M, 0)
        safe = n.clamp(min=1.0)[:, None]
        mean = s1 / safe
        var = s2 / safe - mean ** 2
        sign = torch.where(torch.arange(G, device=s1.device) % 2 == 0, -1.0, 1.0).to(torch.float64)[:, None]
        few = (n < 2)[:, None]
        mean, var = torch.where(few, cmean + sign * SPLIT * cvar.sqrt(), mean), torch.where(few, cvar, var)
        var = torch.maximum(torch.maximum(var, self.var_floor * gvar), torch.full_like(var, VAR_MIN))
        return self._model(mean, var, (n.view(C, M) + 1.0) / (nc[:, None] + M), M)

    def _model(self, mean: torch.Tensor, var: torch.Tensor, weight: Optional[torch.Tensor] = None, mixtures: int = 1) -> Dict:
        """A model's dictionary.  A multi-state model says so, and "mixtures" comes with the weights [C, M]; a 1-state model of
        single Gaussians stays the dictionary it always was."""
        model = {"mean": mean, "var": var, "K": self.K, "n_classes": self.n_classes}
        if self.states > 1:
            model["states"] = self.states
        if weight is not None:
            model.update(weight=weight, mixtures=int(mixtures))
        return model

    # ---- one batch on the device -------------------------------------------------------------------------------------------------
    def _pack(self, mels, ids, optional_ids: Iterable[int], feats) -> Dict:
        dev = self.device
        x = mels if feats is None else feats
        nt, np_ = [int(m.shape[0]) for m in x], [int(t.shape[0]) for t in ids]
        coff_h = kk.packed_offsets([code_words(p, t, self.states) for p, t in zip(np_, nt)])
        tok_h = torch.cat([t.to("cpu", torch.int64) for t in ids])
        opt_h = torch.isin(tok_h, torch.tensor(sorted(set(int(o) for o in optional_ids)), dtype=torch.int64))
        pk = {"B": len(ids), "frames": nt, "tokens": np_,
              "foff": kk.packed_offsets(nt, torch.int32, dev), "poff": kk.packed_offsets(np_, torch.int32, dev),
              "coff": coff_h.to(dev), "coff_host": coff_h.tolist(), "foff_host": kk.packed_offsets(nt).tolist(),
              "poff_host": kk.packed_offsets(np_).tolist(), "ids_host": tok_h, "ids": tok_h.to(torch.int32).to(dev),
              "opt": opt_h.to(torch.uint8).to(dev), "threads": (max(np_) + 63) // 64 * 64}
        packed = torch.cat([m.to(dev, torch.float32) for m in x]).contiguous()
        pk["feat"] = self._features_packed(packed, pk["foff"], pk["B"]) if feats is None else packed.t().contiguous()
        return pk

    def _align_packed(self, pk: Dict, model: Dict) -> Dict:
        dev, B = self.device, pk["B"]
        L = self.loglik(pk["feat"], model)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        end = torch.empty(B, dtype=torch.int32, device=dev)
        codes = torch.empty(pk["coff_host"][-1], dtype=torch.int32, device=dev)
        durations = torch.empty(pk["poff_host"][-1], dtype=torch.int32, device=dev)
        label = torch.empty(pk["foff_host"][-1], dtype=torch.int32, device=dev)
        run = {"feat": pk["feat"], "L": L, "score": score, "end": end, "codes": codes, "durations": durations, "label": label,
               "foff_host": pk["foff_host"], "poff_host": pk["poff_host"], "coff_host": pk["coff_host"],
               "ids": pk["ids"], "foff": pk["foff"], "poff": pk["poff"]}
        S = self.states
        sdur = torch.empty(pk["poff_host"][-1], S, dtype=torch.int32, device=dev) if S > 1 else None      # (1 state: the durations)
        kk.call("kk_align_viterbi", L, L.shape[1], pk["ids"], pk["opt"], pk["foff"], pk["poff"], pk["coff"], B, pk["threads"], S, score,
                end, codes)
        kk.call("kk_align_backtrack", codes, pk["coff"], pk["foff"], pk["poff"], pk["ids"], end, B, S, sdur, durations, label)
        if sdur is not None:
            # label is the class v S + j of every frame (what accumulate takes); the scores take the phoneme: label // S, -1 staying -1
            run.update(states=S, state_durations=sdur, phone_label=torch.div(label, S, rounding_mode="floor"))
        return run

    def run_packed(self, mels: Optional[Sequence[torch.Tensor]], ids: Sequence[torch.Tensor], optional_ids: Iterable[int] = (),
                   model: Optional[Dict] = None, feats: Optional[Sequence[torch.Tensor]] = None) -> Dict:
        """One batch on the device, nothing read back: the features [D, T_total], L [V, T_total], score fp32 [B], end int32 [B] (the
        end state, -1 when infeasible), the code words, durations int32 [P_total], label int32 [T_total] and the host lists foff_host /
        poff_host / coff_host (first frame / token / code word of each utterance), with the packed ids and the offsets foff / poff
        (int32) as the kernels took them.  feats: features [T, D] per utterance instead of mels (then mels is None).  With states = S
        > 1: L is [V S, T_total], end the end TOKEN, label the class v S + j of every frame, and the result also has "states",
        state_durations int32 [P_total, S] (durations are their row sums) and phone_label = label // S."""
        if model is None:
            raise ValueError("run_packed needs a model: fit one, or load one")
        self._check(mels, ids, feats)
        self._check_model(model, self.dim if feats is None else int(feats[0].shape[1]))
        return self._align_packed(self._pack(mels, ids, optional_ids, feats), model)

    @staticmethod
    def _records(run: Dict) -> List[Dict]:
        score, poff, sdur = run["score"].cpu().tolist(), run["poff_host"], None
        if "state_durations" in run:                                             # the phone durations are the row sums: not read
            sdur = run["state_durations"].cpu().to(torch.int64)
            dur = sdur.sum(1)
        else:
            dur = run["durations"].cpu().to(torch.int64)
        out = []
        for n, s in enumerate(score):
            ok = s > -math.inf
            out.append({"durations": dur[poff[n]:poff[n + 1]].clone() if ok else None, "score": s, "feasible": ok})
            if sdur is not None:
                out[-1]["state_durations"] = sdur[poff[n]:poff[n + 1]].clone() if ok else None
        return out

    def align(self, mels: Optional[Sequence[torch.Tensor]], ids: Sequence[torch.Tensor], optional_ids: Iterable[int] = (),
              model: Optional[Dict] = None, feats: Optional[Sequence[torch.Tensor]] = None) -> List[Dict]:
        """mels: log-mels [T, M], ids: integer tokens [P], utterance i = (mels[i], ids[i]); optional_ids: the phoneme ids whose tokens
        may get no frame.  Returns per utterance {"durations": LongTensor [P] summing to T (0 for a skipped token) | None, "score":
        the log-likelihood of the best path, "feasible": whether a path exists}, and with states = S > 1 "state_durations": LongTensor
        [P, S] whose rows sum to the durations (every state of a token that has frames has at least one) | None.  One read of the
        scores and one of the durations by the host."""
        return self._records(self.run_packed(mels, ids, optional_ids, model, feats))

    # ---- pronunciation scores ------------------------------------------------------------------------------------------------------
    def score_packed(self, run: Dict) -> Dict:
        """The pronunciation scores (align_torch.scores) of a run_packed() result, on the device, nothing read back: per token
        gop_sum, lpost_sum (fp64 [P_total]) and hits (int32 [P_total]); per utterance utt_gop, utt_lpost (fp64 [B]) and utt_hits (int32
        [B]); per frame the scratch margin, lpost (fp64 [T_total]) and amax (int32 [T_total]).  Zeros for an infeasible utterance.
        A run of S > 1 states is scored on the phonemes: L is the maximum over each phoneme's states (exact; "phone_L" [V, T_total] in
        the result), the labels are phone_label: another state of the same phoneme winning a frame is no pronunciation error."""
        L, foff, poff = run["L"], run["foff_host"], run["poff_host"]
        S, label = int(run.get("states", 1)), run["label"]
        if S > 1:
            if L.dim() != 2 or L.shape[0] % S:
                raise ValueError(f"L {tuple(L.shape)} does not hold {S} states per phoneme")
            L, label = L.view(L.shape[0] // S, S, L.shape[1]).amax(1).contiguous(), run["phone_label"].contiguous()
            run = dict(run, L=L, label=label)
        if L.dim() != 2 or L.dtype != torch.float32 or not (1 <= L.shape[0] <= MAX_CLASSES):
            raise ValueError(f"L must be fp32 [V <= {MAX_CLASSES}, frames], not {L.dtype} {tuple(L.shape)}")
        B, T_total, P_total = len(foff) - 1, int(L.shape[1]), int(run["ids"].shape[0])
        if B < 1 or len(poff) != B + 1 or foff[-1] != T_total or poff[-1] != P_total:
            raise ValueError(f"the offsets end at {foff[-1]} frames and {poff[-1]} tokens in {B} utterances; L has {T_total} frames and "
                             f"there are {P_total} tokens")
        for k, n in (("label", T_total), ("durations", P_total), ("foff", B + 1), ("poff", B + 1)):
            if tuple(run[k].shape) != (n,) or run[k].dtype != torch.int32:
                raise ValueError(f"{k} must be int32 [{n}], not {run[k].dtype} {tuple(run[k].shape)}")
        if run["ids"].dtype != torch.int32:
            raise ValueError(f"ids must be int32 [{P_total}], not {run['ids'].dtype}")
        limit = max_tokens()
        for n in range(B):
            P, T = poff[n + 1] - poff[n], foff[n + 1] - foff[n]
            if not (1 <= P <= limit):
                raise ValueError(f"utterance {n}: {P} tokens; at most {limit}")
            if not (1 <= T <= MAX_FRAMES):
                raise ValueError(f"utterance {n}: {T} frames; at most {MAX_FRAMES}")
        dev = L.device
        out = {"margin": torch.empty(T_total, dtype=torch.float64, device=dev), "lpost": torch.empty(T_total, dtype=torch.float64, device=dev),
               "amax": torch.empty(T_total, dtype=torch.int32, device=dev),
               "gop_sum": torch.empty(P_total, dtype=torch.float64, device=dev), "lpost_sum": torch.empty(P_total, dtype=torch.float64, device=dev),
               "hits": torch.empty(P_total, dtype=torch.int32, device=dev),
               "utt_gop": torch.empty(B, dtype=torch.float64, device=dev), "utt_lpost": torch.empty(B, dtype=torch.float64, device=dev),
               "utt_hits": torch.empty(B, dtype=torch.int32, device=dev)}
        if S > 1:
            out["phone_L"] = L
        kk.call("kk_align_scores", L, T_total, L.shape[0], run["label"], run["durations"], run["ids"], run["foff"], run["poff"], B,
                out["margin"], out["lpost"], out["amax"], out["gop_sum"], out["lpost_sum"], out["hits"], out["utt_gop"], out["utt_lpost"],
                out["utt_hits"])
        return out

    def score(self, mels: Optional[Sequence[torch.Tensor]], ids: Sequence[torch.Tensor], optional_ids: Iterable[int] = (),
              model: Optional[Dict] = None, feats: Optional[Sequence[torch.Tensor]] = None) -> List[Dict]:
        """align(), and how well every utterance's frames fit the phonemes they were aligned to.  Per utterance {"score", "feasible",
        "durations" as align gives them; "gop": the mean over its frames of L(forced phone) - L(best phone) (<= 0, the classical goodness
        of pronunciation), "logpost": the mean log posterior of the forced phone under a flat prior, "phone_acc": the share of frames
        whose best phone is the forced one; "gop_min", "gop_min_token": the lowest token mean of gop and its index (tokens without frames
        are ignored, the first of equal minima wins); "tokens": {"frames", "hits" int64 [P], "gop", "logpost" fp64 [P], NaN where a
        token has no frames}}; with states = S > 1 also "state_durations" [P, S].  An infeasible utterance has None in every field but
        score and feasible.  One read by the host."""
        run = self.run_packed(mels, ids, optional_ids, model, feats)
        sc = self.score_packed(run)
        parts = [run["score"], run["durations"], sc["gop_sum"], sc["lpost_sum"], sc["hits"], sc["utt_gop"], sc["utt_lpost"], sc["utt_hits"]]
        if "state_durations" in run:
            parts.append(run["state_durations"].reshape(-1))
        host = torch.cat([p.to(torch.float64) for p in parts]).cpu()              # (fp32 and int32 are exact in fp64) the one read
        score, dur, gsum, lsum, hits, ug, ul, uh, *rest = host.split([int(p.shape[0]) for p in parts])
        sdur = rest[0].to(torch.int64).view(-1, run["states"]) if rest else None
        poff, foff, out = run["poff_host"], run["foff_host"], []
        for n, s in enumerate(score.tolist()):
            rec = {"score": s, "feasible": s > -math.inf}
            if not rec["feasible"]:
                rec.update(dict.fromkeys(("durations", "gop", "logpost", "phone_acc", "gop_min", "gop_min_token", "tokens")))
                if sdur is not None:
                    rec["state_durations"] = None
                out.append(rec)
                continue
            sl, T = slice(poff[n], poff[n + 1]), foff[n + 1] - foff[n]
            frames = dur[sl].to(torch.int64)
            nan = torch.full_like(gsum[sl], math.nan)
            tok = {"frames": frames, "gop": torch.where(frames > 0, gsum[sl] / frames, nan),
                   "logpost": torch.where(frames > 0, lsum[sl] / frames, nan), "hits": hits[sl].to(torch.int64)}
            low = torch.where(frames > 0, tok["gop"], torch.full_like(nan, math.inf))
            at = int((low == low.min()).nonzero()[0])                                # (the first of equal minima)
            rec.update(durations=frames.clone(), gop=float(ug[n]) / T, logpost=float(ul[n]) / T, phone_acc=float(uh[n]) / T,
                       gop_min=float(low[at]), gop_min_token=at, tokens=tok)
            if sdur is not None:
                rec["state_durations"] = sdur[sl].clone()
            out.append(rec)
        return out

    def fit(self, mels: Optional[Sequence[torch.Tensor]], ids: Sequence[torch.Tensor], optional_ids: Iterable[int] = (), iters: int = 6,
            batch_size: int = 64, feats: Optional[Sequence[torch.Tensor]] = None, mix_iters: int = 4, on_mix_pass=None):
        """Viterbi training from the even split: `iters` passes of estimate -> align over the corpus in batches of batch_size, the
        class statistics accumulated batch by batch in that order; stops once no duration changes.  Returns (model, durations: list of
        LongTensor [P] | None, scores: the corpus score of each pass).  With states = S > 1 the flat start spreads every token's frames
        of the even split evenly over its S states (flat_start), the passes stop once no STATE duration changes, and the
        state durations of the last pass are in `self.state_durations` (list of LongTensor [P, S] | None).
        With mixtures = M > 1 that training runs first, all of it, with one Gaussian per class; then, for each doubling 1 -> 2 (-> 4),
        every component is split in two (split) and up to mix_iters passes follow, each: align with the current model, assign every
        frame to a component of its class (mix_labels), accumulate batch by batch, estimate (estimate_mix).  A doubling's passes stop
        once no state duration and no count changes.  One closing alignment with the last estimate gives the durations returned, so
        that they are the model's own; `scores` gains one entry per mixture alignment, the closing one included.  on_mix_pass(model,
        runs), if given, is called with every mixture alignment's model and its batches' run_packed() results."""
        if int(iters) != iters or iters < 1:
            raise ValueError(f"iters must be an integer >= 1, not {iters!r}")
        if int(mix_iters) != mix_iters or mix_iters < 1:
            raise ValueError(f"mix_iters must be an integer >= 1, not {mix_iters!r}")
        if int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"batch_size must be an integer >= 1, not {batch_size!r}")
        self._check(mels, ids, feats)
        x = mels if feats is None else feats
        packs = []
        for s in range(0, len(ids), batch_size):
            e = s + batch_size
            packs.append(self._pack(None if feats is not None else x[s:e], ids[s:e], optional_ids, None if feats is None else x[s:e]))
        flat = [torch.from_numpy(even_split(int(t.shape[0]), int(m.shape[0]))) for m, t in zip(x, ids)]
        if self.mixtures > 1:
            return self._fit_mix(packs, flat, int(iters), int(mix_iters), on_mix_pass)
        return self._fit_single(packs, flat, int(iters))

    def _stage(self, mixtures: int) -> "PhoneAligner":
        """This aligner with another number of components (fit's stages 1 -> 2 -> 4), on the same tables."""
        if mixtures == self.mixtures:
            return self
        al = PhoneAligner(self.device, self.K, self.n_classes, self.var_floor, self.states, mixtures)
        al._tables = self._tables
        return al

    @staticmethod
    def _same(old, new) -> bool:
        return all((d is None and e is None) or (d is not None and e is not None and torch.equal(d.reshape(-1), e.reshape(-1)))
                   for d, e in zip(old, new))

    def _align_corpus(self, packs, model, keep_runs: bool = False):
        """One alignment of every batch: (the batches' runs if they are to be kept, the frame labels per batch, what has to stop
        changing per utterance (1 state: the durations), the phone durations per utterance, the corpus score)."""
        runs, labels, new, phone, total = [], [], [], [], 0.0
        for pk in packs:
            run = self._align_packed(pk, model)
            labels.append(run["label"])
            if keep_runs:
                runs.append(run)
            for r in self._records(run):
                new.append(r.get("state_durations", r["durations"]))
                phone.append(r["durations"])
                total += r["score"] if r["feasible"] else 0.0
        return runs, labels, new, phone, total

    def _fit_mix(self, packs, flat, iters: int, mix_iters: int, on_mix_pass):
        model, _, scores = self._stage(1)._fit_single(packs, flat, iters)
        durs = phone = None
        m = 1
        while m < self.mixtures:
            m *= 2
            al = self._stage(m)
            model, counts = al.split(model), None
            for _ in range(mix_iters):
                runs, labels, new, phone, total = al._align_corpus(packs, model, on_mix_pass is not None)
                scores.append(total)
                if on_mix_pass is not None:
                    on_mix_pass(model, runs)
                stats = None
                for pk, lab in zip(packs, labels):
                    part = al.accumulate_mix(pk["feat"], al.mix_labels(pk["feat"], model, lab))
                    stats = part if stats is None else tuple(a + b for a, b in zip(stats, part))
                model = al.estimate_mix(*stats, m)
                n = stats[0].cpu()
                same = counts is not None and durs is not None and torch.equal(n, counts) and self._same(durs, new)
                durs, counts = new, n
                if same:
                    break
        runs, _, durs, phone, total = self._align_corpus(packs, model, on_mix_pass is not None)
        scores.append(total)
        if on_mix_pass is not None:
            on_mix_pass(model, runs)
        self.state_durations = durs if self.states > 1 else None
        return model, phone, scores

    def _fit_single(self, packs, flat, iters: int):
        S, labels, n = self.states, [], 0
        durs: List[Optional[torch.Tensor]] = []                                   # state durations [P, S]
        for pk in packs:
            sd, lab = flat_start(pk["ids_host"], torch.cat(flat[n:n + pk["B"]]), S)
            durs.extend(sd.split(pk["tokens"]))
            labels.append(lab.to(torch.int32).to(self.device))
            n += pk["B"]
        phone: List[Optional[torch.Tensor]] = list(flat)
        model, scores = None, []
        for _ in range(int(iters)):
            stats = None
            for pk, lab in zip(packs, labels):
                part = self.accumulate(pk["feat"], lab)
                stats = part if stats is None else tuple(a + b for a, b in zip(stats, part))
            model = self.estimate(*stats)
            _, labels, new, phone, total = self._align_corpus(packs, model)
            scores.append(total)
            same = self._same(durs, new)
            durs = new
            if same:
                break
        self.state_durations = durs if S > 1 else None
        return model, phone, scores

    # ---- the model on disk -------------------------------------------------------------------------------------------------------
    def save(self, model: Dict, path: str) -> None:
        """A multi-state model's file also has "states"; a 1-state model's file stays what it was (a file without the field is S = 1).
        The same holds for "mixtures", with which "weight" [C, M] comes."""
        self._check_tags(model)
        host = lambda k: model[k].detach().to("cpu", torch.float64)
        torch.save(self._model(host("mean"), host("var"), host("weight") if self.mixtures > 1 else None, self.mixtures), path)

    @staticmethod
    def file_states(path: str) -> int:
        """The states per phoneme of a saved model: 1 for a file without the field."""
        return int(torch.load(path, map_location="cpu", weights_only=True).get("states", 1))

    @staticmethod
    def file_mixtures(path: str) -> int:
        """The components per class of a saved model: 1 for a file without the field."""
        return int(torch.load(path, map_location="cpu", weights_only=True).get("mixtures", 1))

    def load(self, path: str) -> Dict:
        m = torch.load(path, map_location="cpu", weights_only=True)
        if int(m["K"]) != self.K or int(m["n_classes"]) != self.n_classes:
            raise ValueError(f"{path}: a model of K = {int(m['K'])}, {int(m['n_classes'])} classes; this aligner has K = {self.K}, "
                             f"{self.n_classes} classes")
        S = int(m.get("states", 1))
        if S != self.states:
            raise ValueError(f"{path}: a model of states = {S}; this aligner has states = {self.states}")
        M = int(m.get("mixtures", 1))
        if M != self.mixtures:
            raise ValueError(f"{path}: a model of mixtures = {M}; this aligner has mixtures = {self.mixtures}")
        weight = m["weight"] if M > 1 else None
        if tuple(m["mean"].shape[:1]) != (self.gaussians,) or tuple(m["var"].shape[:1]) != (self.gaussians,) or \
                (M > 1 and tuple(weight.shape) != (self.classes, M)):
            have, want = f"{path}: a model of {int(m['mean'].shape[0])} Gaussians", f"{self.n_classes} classes of {S} states"
            raise ValueError(f"{have} and weights {tuple(weight.shape)}; {want} and {M} components need {self.gaussians} and "
                             f"({self.classes}, {M})" if M > 1 else f"{have}; {want} need {self.classes}")
        return self._model(m["mean"].to(self.device), m["var"].to(self.device), None if weight is None else weight.to(self.device), M)
