"""Prosody control of synthesis: speed, pitch, energy and forced per-phoneme values (KokoroEngine.generate / generate_batch /
generate_stream(prosody=...)).

The variance adaptor keeps durations, pitch and energy as explicit tensors between the predictors and the decoder, so the controls
go in at two places of the prefill and nowhere in the decode loop: the durations behind the duration predictor
(kk_prosody_durations) and the per-frame pitch / energy in front of the bucket embeddings (kk_prosody_variance, or
kk_prosody_contour when a row carries a frame-level contour: a recording's pitch / energy track).  The definitions
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
_CONTOURS = ("pitch_contour", "energy_contour")
CONTOUR_MAX = 4096                        # source frames (and phonemes) per row: kk_prosody_contour's two LDS tables


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
    pitch / energy: [P] float in [0, 1], the value of every frame of phoneme p, NaN = keep the model's.
    pitch_contour / energy_contour: [S] float in [0, 1], a frame-level source track (a recording's normalised pitch / energy), NaN =
    not given at this frame; contour_durations: [P] int >= 0 with sum S, the source frames of each phoneme (default: durations,
    when every one of them is forced).  Every frame of phoneme p takes the centre-aligned nearest of the phoneme's source frames
    (prosody_torch.contour); scale and shift then transpose the copied value, and it wins over pitch / energy and the model."""
    speed: FloatOrVector = 1.0
    pitch_scale: FloatOrVector = 1.0
    pitch_shift: FloatOrVector = 0.0
    energy_scale: FloatOrVector = 1.0
    energy_shift: FloatOrVector = 0.0
    durations: Optional[Sequence[int]] = None
    pitch: Optional[Sequence[float]] = None
    energy: Optional[Sequence[float]] = None
    pitch_contour: Optional[Sequence[float]] = None
    energy_contour: Optional[Sequence[float]] = None
    contour_durations: Optional[Sequence[int]] = None

    def _get(self, name: str) -> Optional[torch.Tensor]:
        v = getattr(self, name)
        if v is None:
            return None
        try:
            return _vector(v, torch.int64 if name.endswith("durations") else torch.float32)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"prosody {name}: {e}") from None

    def validate(self, P: int) -> "Prosody":
        """Raises ValueError on a length other than P, speed outside [0.25, 4], a negative (or non-finite) scale, a non-finite shift,
        a forced duration below -1, a forced pitch or energy outside [0, 1]; on contour values outside [0, 1], two tracks of
        different lengths, more than 4096 source frames, contour_durations that are negative, do not sum to the tracks' length or are
        neither given nor implied by fully forced durations.  Returns self."""
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
        self.contours(P)
        return self

    def contours(self, P: int):
        """(pitch track [S] or None, energy track [S] or None, source frames per phoneme int64 [P]) of an utterance of P phonemes,
        validated; None when neither track is given."""
        tracks = [self._get(name) for name in _CONTOURS]
        cd = self._get("contour_durations")
        if tracks[0] is None and tracks[1] is None:
            if cd is not None:
                raise ValueError("prosody contour_durations: given without a pitch_contour or an energy_contour")
            return None
        for name, t in zip(_CONTOURS, tracks):
            if t is None:
                continue
            if t.dim() != 1:
                raise ValueError(f"prosody {name}: a vector of frames is expected")
            if not bool((torch.isnan(t) | ((t >= 0) & (t <= 1))).all()):
                raise ValueError(f"prosody {name} must be in [0, 1], or NaN where it is not given")
        S = int((tracks[0] if tracks[0] is not None else tracks[1]).numel())
        if tracks[0] is not None and tracks[1] is not None and tracks[0].numel() != tracks[1].numel():
            raise ValueError(f"prosody pitch_contour and energy_contour differ in length: {tracks[0].numel()} and {tracks[1].numel()} frames")
        if S > CONTOUR_MAX:
            raise ValueError(f"prosody contour: {S} source frames exceed the limit of {CONTOUR_MAX}")
        if cd is None:
            cd = self._get("durations")
            if cd is None or cd.dim() != 1 or bool((cd < 0).any()):
                raise ValueError("prosody contour_durations: needed unless durations forces every phoneme (no -1)")
        if cd.dim() != 1 or cd.numel() != P:
            raise ValueError(f"prosody contour_durations: a vector of {P} values is expected, one per phoneme")
        if bool((cd < 0).any()):
            raise ValueError("prosody contour_durations must be >= 0")
        if int(cd.sum()) != S:
            raise ValueError(f"prosody contour_durations sum to {int(cd.sum())}, the contour has {S} frames")
        return tracks[0], tracks[1], cd

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
        for name in _CONTOURS:                                # (a track of NaNs alone gives nothing)
            t = self._get(name)
            if t is not None and not bool(torch.isnan(t).all()):
                return False
        return True

    @classmethod
    def from_tracks(cls, durations, pitch=None, energy=None, force_durations: bool = True, **kw) -> "Prosody":
        """The controls that carry a recording's prosody: `durations` [P] frames per phoneme and the normalised frame-level pitch /
        energy tracks, as a feature-cache entry (or FeatureExtractor.extract + PhoneAligner.align) holds them.  A track longer than
        sum(durations) is cut and a shorter one padded with NaN, like the training targets.  force_durations=False keeps the
        model's durations and carries the contour onto them.  kw: further fields (scales, shifts, ...)."""
        d = _vector(durations, torch.int64)
        if d.dim() != 1 or bool((d < 0).any()):
            raise ValueError("prosody from_tracks: durations must be a vector of frames >= 0")
        S = int(d.sum())

        def fit(t):
            if t is None:
                return None
            t = _vector(t, torch.float32).reshape(-1)[:S]
            return torch.cat([t, torch.full((S - t.numel(),), math.nan)])

        return cls(durations=d if force_durations else None, pitch_contour=fit(pitch), energy_contour=fit(energy),
                   contour_durations=d if (pitch is not None or energy is not None) else None, **kw)

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
            if k in ("pitch", "energy") + _CONTOURS and isinstance(v, (list, tuple)):
                v = [math.nan if x is None else x for x in v]
            if k in _FORCED + ("contour_durations",) and not isinstance(v, (list, tuple)):
                raise ValueError(f"prosody {k}: a list of {P} values is expected")
            if k in _CONTOURS and not isinstance(v, (list, tuple)):
                raise ValueError(f"prosody {k}: a list of frames is expected")
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


class PackedContours(NamedTuple):
    """The frame-level source tracks of a batch, what kk_prosody_contour reads next to PackedProsody's tables."""
    pitch: Optional[torch.Tensor]     # [B, Sn] fp32, NaN = not given; None: no row has a pitch track
    energy: Optional[torch.Tensor]    # [B, Sn] fp32, NaN = not given; None: no row has an energy track
    src_dur: torch.Tensor             # [B, Pn] int32, the source frames of each phoneme; 0 on rows without a contour and on padding


def pack_contours(prosody: Optional[Sequence[Optional[Prosody]]], lens_p: Sequence[int], Pn: int, device="cpu") -> Optional[PackedContours]:
    """The contours of a batch as dense tables, Sn = the longest track; None when no row carries one (then the prefill launches what
    it launches without contours).  Every entry is validated against its row's length; ValueError beyond 4096 phonemes."""
    rows = {}
    for b, (pr, n) in enumerate(zip(prosody or (), lens_p)):
        if pr is None:
            continue
        try:
            c = pr.contours(int(n))
        except ValueError as e:
            raise ValueError(f"utterance {b}: {e}") from None
        if c is not None and c[2].sum() > 0:
            rows[b] = c
    if not rows:
        return None
    if Pn > CONTOUR_MAX:
        raise ValueError(f"prosody contour: {Pn} phonemes exceed the limit of {CONTOUR_MAX}")
    B, Sn = len(lens_p), max(int(c[2].sum()) for c in rows.values())
    tracks = [torch.full((B, Sn), math.nan) if any(c[i] is not None for c in rows.values()) else None for i in (0, 1)]
    sd = torch.zeros(B, Pn, dtype=torch.int32)
    for b, c in rows.items():
        sd[b, :c[2].numel()] = c[2].to(torch.int32)
        for i in (0, 1):
            if c[i] is not None:
                tracks[i][b, :c[i].numel()] = c[i]
    return PackedContours(*(t.contiguous().to(device) if t is not None else None for t in (tracks[0], tracks[1], sd)))


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
