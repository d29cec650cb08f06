"""Batched mel synthesis from a trained checkpoint: the engine-side counterpart of the reference's
`KokoroTTS.text_to_speech` / `batch_text_to_speech` (inference/inference.py:489-669), which decode one chunk at a time at B = 1.

`synthesize` sorts the utterances by phoneme count and runs `KokoroEngine.generate_batch` on batches of them; every mel equals
what the B = 1 path gives that utterance alone.  `load_for_inference` builds an engine from a `kokoro-train` checkpoint and
resolves the inference controls as the reference's loader does.  Text -> phonemes and the vocoder stay on the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

DEFAULT_CONTROLS = {"max_len": 1200, "stop_threshold": 0.45, "min_len_ratio": 0.7, "min_len_floor": 12}   # inference.py:395-400


@dataclass
class InferenceControls:
    """The keyword arguments of generate / generate_batch a checkpoint decides (inference.py:393-452, 552-562)."""
    max_len: int = 1200
    stop_threshold: float = 0.45
    min_len_ratio: float = 0.7
    min_len_floor: int = 12
    post_expected_stop_threshold: Optional[float] = None     # None: the model's default (0.2)

    def kwargs(self) -> Dict[str, Any]:
        kw = dict(max_len=self.max_len, stop_threshold=self.stop_threshold, min_len_ratio=self.min_len_ratio,
                  min_len_floor=self.min_len_floor)
        if self.post_expected_stop_threshold is not None:
            kw["post_expected_stop_threshold"] = self.post_expected_stop_threshold
        return kw


def _safe_float(value: Any, default: float, min_value: float, max_value: float) -> float:      # inference.py:376-382
    try:
        value_f = float(value)
    except (TypeError, ValueError):
        return default
    return max(min_value, min(max_value, value_f))


def _safe_int(value: Any, default: int, min_value: int) -> int:                                # inference.py:384-390
    try:
        value_i = int(value)
    except (TypeError, ValueError):
        return default
    return max(min_value, value_i)


def resolve_controls(checkpoint: Dict[str, Any], max_len: Optional[int] = None, stop_threshold: Optional[float] = None,
                     min_len_ratio: Optional[float] = None, min_len_floor: Optional[int] = None) -> InferenceControls:
    """_apply_checkpoint_inference_controls (inference.py:393-452): each control is metadata `inference_controls` -> config field
    `inference_*` -> default, clamped; an explicit argument wins unclamped.  An explicit stop threshold is also the
    post-expected-length threshold (inference.py:552-562), so a lower model default does not override it."""
    meta = checkpoint.get("model_metadata", {}) if isinstance(checkpoint, dict) else {}
    mc = meta.get("inference_controls", {}) if isinstance(meta, dict) else {}
    mc = mc if isinstance(mc, dict) else {}
    cfg = checkpoint.get("config") if isinstance(checkpoint, dict) else None
    cc = {}
    if cfg is not None:
        cc = {k: getattr(cfg, f"inference_{k}", None) for k in DEFAULT_CONTROLS}
    chosen = {k: mc.get(k, cc.get(k, DEFAULT_CONTROLS[k])) for k in DEFAULT_CONTROLS}
    c = InferenceControls(
        max_len=int(max_len) if max_len is not None else _safe_int(chosen["max_len"], DEFAULT_CONTROLS["max_len"], min_value=64),
        stop_threshold=(float(stop_threshold) if stop_threshold is not None else
                        _safe_float(chosen["stop_threshold"], DEFAULT_CONTROLS["stop_threshold"], min_value=0.05, max_value=0.99)),
        min_len_ratio=(float(min_len_ratio) if min_len_ratio is not None else
                       _safe_float(chosen["min_len_ratio"], DEFAULT_CONTROLS["min_len_ratio"], min_value=0.1, max_value=1.5)),
        min_len_floor=(int(min_len_floor) if min_len_floor is not None else
                       _safe_int(chosen["min_len_floor"], DEFAULT_CONTROLS["min_len_floor"], min_value=1)))
    if stop_threshold is not None:
        c.post_expected_stop_threshold = c.stop_threshold
    return c


def pick_weights(checkpoint: Dict[str, Any], weights: str = "auto") -> Tuple[Dict[str, torch.Tensor], str]:
    """KokoroTTS._load_model's choice of state dict (inference.py:154-191): `auto` prefers the EMA weights, `ema` requires them,
    `model` takes model_state_dict (or `model`, or the checkpoint itself as a raw state dict)."""
    if weights not in ("auto", "ema", "model"):
        raise ValueError(f"weights must be auto, ema or model, not {weights!r}")
    sd = checkpoint.get("model_state_dict", checkpoint.get("model", checkpoint))
    if weights in ("auto", "ema") and "ema_model_state_dict" in checkpoint:
        return checkpoint["ema_model_state_dict"], "ema"
    if weights == "ema":
        raise RuntimeError("EMA weights requested but 'ema_model_state_dict' not found in checkpoint.")
    return sd, "model"


def dims_from_checkpoint(checkpoint: Dict[str, Any], state_dict: Dict[str, torch.Tensor]):
    """ModelDims of a checkpoint: its architecture metadata, the vocabulary from the embedding table."""
    from kokoro_ruslan_amd.spec import ModelDims
    arch = (checkpoint.get("model_metadata") or {}).get("architecture") or {}
    dflt = ModelDims()
    g = lambda k, d: int(arch.get(k, d))
    return ModelDims(vocab=int(state_dict["text_embedding.weight"].shape[0]), mel=g("mel_dim", dflt.mel), hidden=g("hidden_dim", dflt.hidden),
                     heads=g("n_heads", dflt.heads), enc_layers=g("n_encoder_layers", dflt.enc_layers),
                     dec_layers=g("n_decoder_layers", dflt.dec_layers), enc_ff=g("encoder_ff_dim", dflt.enc_ff),
                     dec_ff=g("decoder_ff_dim", dflt.dec_ff), var_filter=g("variance_filter_size", dflt.var_filter),
                     var_kernel=g("variance_kernel_size", dflt.var_kernel), var_bins=g("n_variance_bins", dflt.var_bins),
                     max_len=g("max_decoder_seq_len", dflt.max_len))


def load_for_inference(path: str, weights: str = "auto", device: str = "cuda", math_mode: str = "f32",
                       max_len: Optional[int] = None, stop_threshold: Optional[float] = None, min_len_ratio: Optional[float] = None,
                       min_len_floor: Optional[int] = None):
    """(engine, InferenceControls, weights used) from a checkpoint written by kokoro-train."""
    from kokoro.training.checkpoint import check_metadata
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import StepHyper
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd, used = pick_weights(ckpt, weights)
    dims = dims_from_checkpoint(ckpt, sd)
    check_metadata(ckpt, dims)
    eng = KokoroEngine(dims, StepHyper(), device=device, math_mode=math_mode, init=False)
    eng.load_state_dict(sd, strict=True)
    return eng, resolve_controls(ckpt, max_len, stop_threshold, min_len_ratio, min_len_floor), used


def synthesize(engine, utterances: Sequence[torch.Tensor], stress: Optional[Sequence[torch.Tensor]] = None, batch_size: int = 32,
               stream: bool = False, slots: int = 32, prosody=None, **stop_kwargs) -> List[torch.Tensor]:
    """Mels [frames_b, n_mels] of every utterance, in input order.  Utterances are sorted by phoneme count and decoded
    `batch_size` at a time by engine.generate_batch (sorting keeps the padding and the shared length bound of a batch small).
    stream=True decodes them all in one engine.generate_stream call instead: a pool of `slots` rows in which a finished row's
    slot is refilled with the next utterance (continuous batching; input order, no sorting, batch_size unused).
    prosody: one kokoro_ruslan_amd.prosody.Prosody for every utterance, or one per utterance in input order (None entries: neutral);
    each batch is handed its utterances' controls.  None: no controls, the engine is called as without the argument."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    if stress is not None and len(stress) != len(utterances):
        raise ValueError(f"stress: {len(stress)} vectors for {len(utterances)} utterances")
    if prosody is not None:
        from kokoro_ruslan_amd.prosody import as_list
        prosody = as_list(prosody, len(utterances))
    if stream:
        if slots < 1:
            raise ValueError("slots must be >= 1")
        if prosody is not None:
            stop_kwargs = dict(stop_kwargs, prosody=prosody)
        return list(engine.generate_stream(list(utterances), list(stress) if stress is not None else None, slots=slots, **stop_kwargs))
    order = sorted(range(len(utterances)), key=lambda i: (int(utterances[i].numel()), i))
    out: List[Optional[torch.Tensor]] = [None] * len(utterances)
    for s in range(0, len(order), batch_size):
        part = order[s:s + batch_size]
        kw = stop_kwargs if prosody is None else dict(stop_kwargs, prosody=[prosody[i] for i in part])
        mels = engine.generate_batch([utterances[i] for i in part], [stress[i] for i in part] if stress is not None else None,
                                     **kw)
        for i, m in zip(part, mels):
            out[i] = m
    return out


def trim_trailing_silence(mel: torch.Tensor) -> torch.Tensor:
    """The reference's clamp and trailing-silence trim before vocoding (inference.py:588-619) on one mel [frames, n_mels]."""
    mel = torch.clamp(mel, min=-11.5, max=2.0)                                      # :590
    frame_means = mel.mean(dim=-1)                                                   # :596
    if frame_means.numel() == 0:                                                     # :597
        return mel
    q10 = float(torch.quantile(frame_means, 0.10).item())                            # :599
    q20 = float(torch.quantile(frame_means, 0.20).item())                            # :600
    adaptive_threshold = max(-9.8, min(-9.2, 0.5 * (q10 + q20)))                     # :601
    voiced = (frame_means > adaptive_threshold).nonzero(as_tuple=False).squeeze(-1)  # :603
    if voiced.numel() == 0:                                                          # :604 (else: no trim, :618-619)
        return mel
    last_voiced = int(voiced[-1].item())                                             # :605
    trailing_margin, min_keep_frames = 24, 60                                        # :609-610
    proposed_end = min(mel.shape[0], last_voiced + trailing_margin + 1)              # :612
    t_end = max(min_keep_frames, proposed_end)                                       # :613
    t_end = min(t_end, mel.shape[0])                                                 # :614
    return mel[:t_end]                                                               # :616
