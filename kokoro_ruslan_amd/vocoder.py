"""HiFi-GAN vocoding on the device: a batch of mels [frames_b, 80] to waveforms, on the kernels of csrc/kk_vocoder.hip.

`HifiganVocoder` restates the generator of a HiFi-GAN universal checkpoint (resblock "1", 80 mels): conv_pre, per stage a
leaky_relu(0.1) + ConvTranspose1d and the multi-receptive-field sum of the residual blocks, then leaky_relu(0.01), conv_post, tanh.
The mels of one call are packed back to back along time (utterance starts per stage in a small table, no padding) and run through
~80 launches per group; every conv masks its taps to the utterance, so row b of a batch is, bit for bit, the utterance vocoded
alone.  math_mode "bf16": bf16 operands, fp32 accumulation; "f32": fp32 operands on the fp32 MFMA.  The residual stream and the
multi-receptive-field sum stay fp32 in both.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from kokoro_ruslan_amd import lib as kk

DEFAULT_CONFIG = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
                  "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
                  "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "num_mels": 80, "sampling_rate": 22050}
NUM_MELS = 80
DEFAULT_MAX_SAMPLES = 1 << 23          # packed output samples per group (4 fp32 workspaces of ~32 floats per sample: ~4.3 GB)
_KC, _NB = 32, 64                      # K chunk and output-channel tile of the conv core: the padding of the packed weights


def _up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def convt_taps(k: int, stride: int) -> Tuple[int, int]:
    """(first tap offset, taps) of the polyphase ConvTranspose1d(k, stride, padding (k - stride) / 2): output q * stride + r reads
    input rows q + off0 .. q + off0 + taps - 1 (the same rule as kk_voc_convt_taps)."""
    if stride < 1 or k < stride or (k - stride) % 2:
        raise ValueError(f"ConvTranspose1d(k={k}, stride={stride}): the polyphase form needs k >= stride and k - stride even "
                         "(padding (k - stride) / 2 gives exactly stride samples per input frame)")
    p = (k - stride) // 2
    amin, amax, mmax = p // stride, (p + stride - 1) // stride, -(-k // stride) - 1
    return amin - mmax, amax - (amin - mmax) + 1


def pack_conv(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Conv1d weight [cout, cin, k] -> tap-major [k][npad][kpad] (K = cin contiguous, zero padded)."""
    cout, cin, k = w.shape
    out = torch.zeros(k, _up(cout, _NB), _up(cin, _KC), dtype=dtype, device=w.device)
    out[:, :cout, :cin] = w.permute(2, 0, 1).to(dtype)
    return out


def pack_convt(w: torch.Tensor, stride: int, dtype: torch.dtype) -> torch.Tensor:
    """ConvTranspose1d weight [cin, cout, k] -> the polyphase conv's [taps][npad][kpad]: channel r * cout + co of input row q is output
    sample q * stride + r; tap t (input row q + off0 + t) feeds it through kernel index kk = m * stride + b, where r + p = a * stride + b
    and t + off0 = a - m."""
    cin, cout, k = w.shape
    off0, taps = convt_taps(k, stride)
    p = (k - stride) // 2
    out = torch.zeros(taps, _up(cout * stride, _NB), _up(cin, _KC), dtype=dtype, device=w.device)
    for r in range(stride):
        a, b = divmod(r + p, stride)
        for m in range((k - b + stride - 1) // stride):
            out[a - m - off0, r * cout:(r + 1) * cout, :cin] = w[:, :, m * stride + b].t().to(dtype)
    return out


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g * v / ||v||, the norm over every dim but 0 (torch weight_norm's dim=0; dim 0 of a ConvTranspose1d weight is Cin)."""
    norm = v.norm(2, dim=tuple(range(1, v.dim())), keepdim=True)
    return v * (g / norm)


def resolve_config(config: Optional[dict]) -> dict:
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(config or {})
    if str(cfg.get("resblock", "1")) != "1":
        raise ValueError(f"HiFi-GAN resblock type {cfg['resblock']!r}: only \"1\" is implemented (as in the reference)")
    if int(cfg.get("num_mels", NUM_MELS)) != NUM_MELS:
        raise ValueError(f"num_mels {cfg['num_mels']}: the generator takes {NUM_MELS} mel channels")
    if len(cfg["upsample_rates"]) != len(cfg["upsample_kernel_sizes"]):
        raise ValueError("upsample_rates and upsample_kernel_sizes differ in length")
    if len(cfg["resblock_kernel_sizes"]) != len(cfg["resblock_dilation_sizes"]):
        raise ValueError("resblock_kernel_sizes and resblock_dilation_sizes differ in length")
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        convt_taps(int(k), int(u))
    for k in cfg["resblock_kernel_sizes"]:
        if int(k) % 2 == 0:
            raise ValueError(f"resblock kernel size {k}: must be odd")
    c0 = int(cfg["upsample_initial_channel"])
    if c0 % (1 << len(cfg["upsample_rates"])) or (c0 >> len(cfg["upsample_rates"])) % 4:
        raise ValueError(f"upsample_initial_channel {c0}: every stage's channel count must be a multiple of 4")
    return cfg


def layer_shapes(cfg: dict) -> Dict[str, Tuple[str, Tuple[int, ...]]]:
    """name -> (kind, weight shape) of the generator's convolutions, in the order of its state dict."""
    c0, nk = int(cfg["upsample_initial_channel"]), len(cfg["resblock_kernel_sizes"])
    out = {"conv_pre": ("conv", (c0, NUM_MELS, 7))}
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        out[f"ups.{i}"] = ("convt", (c0 >> i, c0 >> (i + 1), int(k)))
    for i in range(len(cfg["upsample_rates"])):
        ch = c0 >> (i + 1)
        for j, (k, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            for part in ("convs1", "convs2"):
                for m in range(len(ds)):
                    out[f"resblocks.{i * nk + j}.{part}.{m}"] = ("conv", (ch, ch, int(k)))
    out["conv_post"] = ("conv", (1, c0 >> len(cfg["upsample_rates"]), 7))
    return out


def load_config(path: Optional[str]) -> dict:
    if path is None:
        return dict(DEFAULT_CONFIG)
    with open(path) as f:
        return json.load(f)


class HifiganVocoder:
    """Batched HiFi-GAN generator on the MI355X.  load_state_dict / from_checkpoint, then vocode(list of [frames_b, 80] mels)."""

    def __init__(self, config: Optional[dict] = None, device: str = "cuda", math_mode: str = "bf16"):
        if math_mode not in ("bf16", "f32"):
            raise ValueError(f"math_mode must be bf16 or f32, not {math_mode!r}")
        self.config = resolve_config(config)
        self.device = torch.device(device)
        self.math_mode = math_mode
        self.rates = [int(u) for u in self.config["upsample_rates"]]
        self.up_kernels = [int(k) for k in self.config["upsample_kernel_sizes"]]
        self.c0 = int(self.config["upsample_initial_channel"])
        self.res_kernels = [int(k) for k in self.config["resblock_kernel_sizes"]]
        self.res_dilations = [[int(d) for d in ds] for ds in self.config["resblock_dilation_sizes"]]
        self.hop = math.prod(self.rates)
        self.sampling_rate = int(self.config.get("sampling_rate", 22050))
        self.shapes = layer_shapes(self.config)
        self.weights: Optional[Dict[str, torch.Tensor]] = None     # folded fp32 weights [as in the checkpoint], on the CPU
        self._packed: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._ws: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Strict: every conv needs its bias and its weight in one of the three forms (weight_g/weight_v,
        parametrizations.weight.original0/original1, or a plain weight); a missing or an unexpected key raises."""
        keys, folded, missing = set(sd), {}, []
        for name, (_, shape) in self.shapes.items():
            forms = ((f"{name}.weight_g", f"{name}.weight_v"),
                     (f"{name}.parametrizations.weight.original0", f"{name}.parametrizations.weight.original1"))
            for gk, vk in forms:
                if gk in sd and vk in sd:
                    w = fold_weight_norm(sd[gk].float(), sd[vk].float())
                    keys -= {gk, vk}
                    break
            else:
                if f"{name}.weight" in sd:
                    w = sd[f"{name}.weight"].float()
                    keys.discard(f"{name}.weight")
                else:
                    missing.append(f"{name}.weight")
                    continue
            if tuple(w.shape) != shape:
                raise ValueError(f"{name}: weight of shape {tuple(w.shape)}, the config needs {shape}")
            if f"{name}.bias" not in sd:
                missing.append(f"{name}.bias")
                continue
            keys.discard(f"{name}.bias")
            folded[name] = (w.detach().cpu().contiguous(), sd[f"{name}.bias"].float().detach().cpu().contiguous())
        if missing or keys:
            raise KeyError(f"HiFi-GAN state dict does not match the config: missing {sorted(missing)[:8]}"
                           f"{' ...' if len(missing) > 8 else ''}, unexpected {sorted(keys)[:8]}{' ...' if len(keys) > 8 else ''}")
        self.weights = {n: w for n, (w, _) in folded.items()}
        self.biases = {n: b for n, (_, b) in folded.items()}
        dt = torch.bfloat16 if self.math_mode == "bf16" else torch.float32
        self._packed = {}
        for i, u in enumerate(self.rates):
            n = f"ups.{i}"
            self._packed[n] = (pack_convt(self.weights[n], u, dt).to(self.device), self.biases[n].to(self.device))
        for n, (kind, _) in self.shapes.items():
            if n == "conv_post":
                w = self.weights[n][0].t().contiguous()                    # [k][cin] fp32
                self._packed[n] = (w.to(self.device), self.biases[n].to(self.device))
            elif kind == "conv":
                self._packed[n] = (pack_conv(self.weights[n], dt).to(self.device), self.biases[n].to(self.device))

    @classmethod
    def from_checkpoint(cls, path: str, config_path: Optional[str] = None, device: str = "cuda",
                        math_mode: str = "bf16") -> "HifiganVocoder":
        """A directory means <dir>/generator.pth + <dir>/config.json; a file means a sibling config.json; no config file means the
        default config.  A top-level 'generator' entry is unwrapped.  Local files only."""
        ckpt, cfg_path = resolve_checkpoint(path, config_path)
        config = load_config(cfg_path)
        sd = torch.load(ckpt, map_location="cpu", weights_only=False)
        if isinstance(sd, dict) and "generator" in sd:
            sd = sd["generator"]
        voc = cls(config, device=device, math_mode=math_mode)
        voc.load_state_dict(sd)
        return voc

    # ------------------------------------------------------------------ forward
    def _workspace(self, floats: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < floats:
            self._ws = None
            self._ws = torch.empty(floats, dtype=torch.float32, device=self.device)
        return self._ws

    def vocode(self, mels: Sequence[torch.Tensor], max_samples: int = DEFAULT_MAX_SAMPLES) -> List[torch.Tensor]:
        """One fp32 waveform of frames_b * prod(upsample_rates) samples per mel [frames_b, 80], in input order.  The mels run in
        groups of at most max_samples packed output samples (a longer mel runs alone)."""
        if not self._packed:
            raise RuntimeError("HifiganVocoder: no weights (load_state_dict or from_checkpoint first)")
        for i, m in enumerate(mels):
            if m.dim() != 2 or m.shape[1] != NUM_MELS or m.shape[0] < 1:
                raise ValueError(f"mel {i}: shape {tuple(m.shape)}, expected [frames >= 1, {NUM_MELS}]")
        out: List[torch.Tensor] = []
        group, total = [], 0
        for m in mels:
            s = m.shape[0] * self.hop
            if group and total + s > max_samples:
                out += self._run(group)
                group, total = [], 0
            group.append(m)
            total += s
        if group:
            out += self._run(group)
        return out

    def _run(self, mels: List[torch.Tensor]) -> List[torch.Tensor]:
        dev, bf = self.device, 1 if self.math_mode == "bf16" else 0
        frames = [int(m.shape[0]) for m in mels]
        T = sum(frames)
        x = torch.cat([m.to(dev, torch.float32) for m in mels]).contiguous()
        nb = len(mels)
        starts = [0]
        for f in frames:
            starts.append(starts[-1] + f)
        mult = [1]
        for u in self.rates:
            mult.append(mult[-1] * u)
        seg = torch.tensor([[s * m for s in starts] for m in mult], dtype=torch.int32).to(dev)      # [stages + 1][B + 1]
        chans = [self.c0 >> i for i in range(len(self.rates) + 1)]
        per = max([T * self.c0] + [T * mult[i + 1] * chans[i + 1] for i in range(len(self.rates))])
        ws = self._workspace(4 * per)
        A, X, H, Tt = (ws[i * per:(i + 1) * per] for i in range(4))
        nk = len(self.res_kernels)

        w, b = self._packed["conv_pre"]
        kk.call("kk_voc_conv1d", x, T, NUM_MELS, w, w.shape[2], w.shape[1], b, A, self.c0, 7, 1, 1.0, seg[0], nb, None, None, 0, bf)
        rows = T
        for i, u in enumerate(self.rates):
            cin, ch = chans[i], chans[i + 1]
            w, b = self._packed[f"ups.{i}"]
            kk.call("kk_voc_convt1d", A, rows, cin, w, w.shape[2], w.shape[1], b, X, ch, self.up_kernels[i], u, 0.1, seg[i], nb, bf)
            rows *= u
            sg = seg[i + 1]
            for j, (k, ds) in enumerate(zip(self.res_kernels, self.res_dilations)):
                base = f"resblocks.{i * nk + j}"
                for m, d in enumerate(ds):
                    last = m == len(ds) - 1
                    w1, b1 = self._packed[f"{base}.convs1.{m}"]
                    kk.call("kk_voc_conv1d", X if m == 0 else H, rows, ch, w1, w1.shape[2], w1.shape[1], b1, Tt, ch, k, d, 0.1, sg, nb,
                            None, None, 0, bf)
                    w2, b2 = self._packed[f"{base}.convs2.{m}"]
                    res = X if m == 0 else H
                    if not last:
                        kk.call("kk_voc_conv1d", Tt, rows, ch, w2, w2.shape[2], w2.shape[1], b2, H, ch, k, 1, 0.1, sg, nb, res, None, 0, bf)
                    else:                            # the resblock's output goes into the multi-receptive-field sum
                        kk.call("kk_voc_conv1d", Tt, rows, ch, w2, w2.shape[2], w2.shape[1], b2, A, ch, k, 1, 0.1, sg, nb, res,
                                A if j > 0 else None, nk if j == nk - 1 else 0, bf)
        w, b = self._packed["conv_post"]
        y = torch.empty(rows, dtype=torch.float32, device=dev)
        kk.call("kk_voc_post", A, rows, chans[-1], w, b, y, 7, 0.01, seg[-1], nb)
        return list(y.split([f * self.hop for f in frames]))


def resolve_checkpoint(path: str, config_path: Optional[str] = None) -> Tuple[str, Optional[str]]:
    """(generator checkpoint, config file or None) the way the reference's vocoder loader finds them."""
    if os.path.isdir(path):
        ckpt = os.path.join(path, "generator.pth")
        sibling = os.path.join(path, "config.json")
    else:
        ckpt = path
        sibling = os.path.join(os.path.dirname(os.path.abspath(path)), "config.json")
    if not os.path.exists(ckpt):
        raise FileNotFoundError(f"HiFi-GAN checkpoint not found: {ckpt}")
    if config_path is None and os.path.exists(sibling):
        config_path = sibling
    if config_path is not None and not os.path.exists(config_path):
        config_path = None                       # the reference falls back to the default config
    return ckpt, config_path
