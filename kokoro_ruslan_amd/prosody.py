"""Prosody control of synthesis: speed, pitch, energy and forced per-phoneme values (KokoroEngine.generate / generate_batch /
generate_stream(prosody=...)).

The variance adaptor keeps durations, pitch and energy as explicit tensors between the predictors and the decoder, so the controls
go in at two places of the prefill and nowhere in the decode loop: the durations behind the duration predictor
(kk_prosody_durations) and the per-frame pitch / energy in front of the bucket embeddings (kk_prosody_variance).  The definitions
are in include/kokoro_hip.h and, restated in fp32 torch, in prosody_torch.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Union

import torch

SPEED_MIN, SPEED_MAX = 0.25, 4.0          # an interface limit, not a measurement
FloatOrVector = Union[float, Sequence[float], torch.Tensor]

_NEUTRAL = {"speed": 1.0, "pitch_scale": 1.0, "pitch_shift": 0.0, "energy_scale": 1.0, "energy_shift": 0.0}
_FORCED = ("durations", "pitch", "energy")


def _vector(v, dtype) -> torch.Tensor:
    """A scalar as a 0-d tensor, a list / array / tensor as a 1-d one, on the host."""
    t = v.detach().to("cpu") if isinstance(v, torch.Tensor) else torch.as_tensor(v)
    if t.dim() > 1:
        raise ValueError(f"a scalar or a vector is expected, not {tuple(t.shape)}")
    if dtype is torch.int64 and t.is_floating_point():
        if not bool(torch.equal(t, t.round())):
            raise ValueError("durations must be whole frames")
    return t.to(dtype)


@dataclass
class Prosody:
    """Controls of one utterance of P phonemes; every field is optional.

    speed: frames per phoneme are divided by it (a phoneme the model gave a frame keeps at least one).  pitch_scale / pitch_shift:
    applied to the clamped normalised pitch of voiced frames; energy_scale / energy_shift: to the clamped normalised energy of every
    frame.  Each is a float or a [P] vector.  durations: [P] int, the frames of phoneme p used as given, -1 = keep the model's.
    pitch / energy: [P] float in [0, 1], the value of every frame of phoneme p, NaN = keep the model's."""
    speed: FloatOrVector = 1.0
    pitch_scale: FloatOrVector = 1.0
    pitch_shift: FloatOrVector = 0.0
    energy_scale: FloatOrVector = 1.0
    energy_shift: FloatOrVector = 0.0
    durations: Optional[Sequence[int]] = None
    pitch: Optional[Sequence[float]] = None
    energy: Optional[Sequence[float]] = None

    def _get(self, name: str) -> Optional[torch.Tensor]:
        v = getattr(self, name)
        if v is None:
            return None
        try:
            return _vector(v, torch.int64 if name == "durations" else torch.float32)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"prosody {name}: {e}") from None

    def validate(self, P: int) -> "Prosody":
        """Raises ValueError on a length other than P, speed outside [0.25, 4], a negative (or non-finite) scale, a non-finite shift,
        a forced duration below -1, a forced pitch or energy outside [0, 1].  Returns self."""
        for name in _NEUTRAL:
            t = self._get(name)
            if t is None:
                raise ValueError(f"prosody {name}: None (leave the field out for its neutral value)")
            if t.dim() == 1 and t.numel() != P:
                raise ValueError(f"prosody {name}: {t.numel()} values for {P} phonemes")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"prosody {name} must be finite")
            if name == "speed" and not bool(((t >= SPEED_MIN) & (t <= SPEED_MAX)).all()):
                raise ValueError(f"prosody speed must be in [{SPEED_MIN}, {SPEED_MAX}]")
            if name.endswith("_scale") and bool((t < 0).any()):
                raise ValueError(f"prosody {name} must be >= 0")
        for name in _FORCED:
            t = self._get(name)
            if t is None:
                continue
            if t.dim() != 1 or t.numel() != P:
                raise ValueError(f"prosody {name}: a vector of {P} values is expected, one per phoneme")
            if name == "durations":
                if bool((t < -1).any()):
                    raise ValueError("prosody durations must be >= 0, or -1 to keep the model's")
                if bool((t > 2 ** 31 - 1).any()):
                    raise ValueError("prosody durations exceed the int32 table")
            else:
                ok = torch.isnan(t) | ((t >= 0) & (t <= 1))
                if not bool(ok.all()):
                    raise ValueError(f"prosody {name} must be in [0, 1], or NaN to keep the model's")
        return self

    def is_neutral(self) -> bool:
        """Every field at its neutral value: nothing scaled, shifted or forced."""
        for name, v in _NEUTRAL.items():
            t = self._get(name)
            if t is None or not bool((t == v).all()):
                return False
        d = self._get("durations")
        if d is not None and bool((d != -1).any()):
            return False
        for name in ("pitch", "energy"):
            t = self._get(name)
            if t is not None and not bool(torch.isnan(t).all()):
                return False
        return True

    @classmethod
    def from_json(cls, obj: Dict[str, Any], P: int) -> "Prosody":
        """From a dict with the fields' names; scalars or lists (null in a forced pitch / energy list = NaN = keep the model's).
        Validated for P phonemes."""
        if not isinstance(obj, dict):
            raise ValueError(f"prosody must be an object, not {type(obj).__name__}")
        known = {f.name for f in fields(cls)}
        unknown = sorted(set(obj) - known)
        if unknown:
            raise ValueError(f"prosody: unknown field(s) {', '.join(unknown)}")
        kw = {}
        for k, v in obj.items():
            if v is None:
                continue
            if k in ("pitch", "energy") and isinstance(v, (list, tuple)):
                v = [math.nan if x is None else x for x in v]
            if k in _FORCED and not isinstance(v, (list, tuple)):
                raise ValueError(f"prosody {k}: a list of {P} values is expected")
            if isinstance(v, (str, bool)) or (isinstance(v, (list, tuple)) and any(isinstance(x, (str, bool)) for x in v)):
                raise ValueError(f"prosody {k}: numbers are expected")
            kw[k] = v
        return cls(**kw).validate(P)


class PackedProsody(NamedTuple):
    """The dense tables of a batch, what the kernels read.  pitch_ss / energy_ss are [2, B, Pn]: plane 0 the scale, plane 1 the shift."""
    speed: torch.Tensor            # [B, Pn] fp32
    pitch_ss: torch.Tensor         # [2, B, Pn] fp32
    energy_ss: torch.Tensor        # [2, B, Pn] fp32
    pitch: torch.Tensor            # [B, Pn] fp32, NaN = not forced
    energy: torch.Tensor           # [B, Pn] fp32, NaN = not forced
    durations: torch.Tensor        # [B, Pn] int32, -1 = not forced


def pack(prosody: Sequence[Optional[Prosody]], lens_p: Sequence[int], Pn: int, device="cpu") -> PackedProsody:
    """Six dense tables of B = len(prosody) rows of Pn phonemes, row b from prosody[b] (None: neutral) over its lens_p[b] phonemes;
    padding positions carry the neutral values.  Every entry is validated against its row's length."""
    B = len(prosody)
    if len(lens_p) != B:
        raise ValueError(f"prosody: {B} entries for {len(lens_p)} utterances")
    if B == 0 or Pn < max(int(n) for n in lens_p):
        raise ValueError("prosody: Pn must cover the longest row of a non-empty batch")
    speed = torch.ones(B, Pn)
    pss, ess = torch.zeros(2, B, Pn), torch.zeros(2, B, Pn)
    pss[0], ess[0] = 1.0, 1.0
    fp, fe = torch.full((B, Pn), math.nan), torch.full((B, Pn), math.nan)
    fd = torch.full((B, Pn), -1, dtype=torch.int32)
    for b, (pr, n) in enumerate(zip(prosody, lens_p)):
        if pr is None:
            continue
        if not isinstance(pr, Prosody):
            raise ValueError(f"prosody: entry {b} is a {type(pr).__name__}, not a Prosody")
        n = int(n)
        try:
            pr.validate(n)
        except ValueError as e:
            raise ValueError(f"utterance {b}: {e}") from None
        for dst, name in ((speed[b], "speed"), (pss[0, b], "pitch_scale"), (pss[1, b], "pitch_shift"), (ess[0, b], "energy_scale"),
                          (ess[1, b], "energy_shift"), (fp[b], "pitch"), (fe[b], "energy"), (fd[b], "durations")):
            t = pr._get(name)
            if t is not None:
                dst[:n] = t.to(dst.dtype)            # (a 0-d tensor broadcasts over the row's phonemes)
    return PackedProsody(*(t.contiguous().to(device) for t in (speed, pss, ess, fp, fe, fd)))


def as_list(prosody, n: int, what: str = "utterances") -> Optional[List[Optional[Prosody]]]:
    """The prosody argument of the entry points as one entry per row: None stays None, one Prosody serves every row, a sequence
    must have n entries (None entries: neutral)."""
    if prosody is None:
        return None
    if isinstance(prosody, Prosody):
        return [prosody] * n
    lst = list(prosody)
    if len(lst) != n:
        raise ValueError(f"prosody: {len(lst)} entries for {n} {what}")
    return lst
