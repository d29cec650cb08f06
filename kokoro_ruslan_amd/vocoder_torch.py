"""The HiFi-GAN generator written with torch.nn.functional on folded weights: the yardstick the vocoder kernels are tested and
benchmarked against (tests/test_vocoder_*.py, tools/vocoder_bench.py).  Not a fallback: HifiganVocoder never calls it.

forward(): one utterance [frames, 80] -> [frames * prod(upsample_rates)] (or a padded batch [B, frames, 80] -> [B, samples]), in the
dtype of the weights given.  round_bf16 rounds the
operand of every MFMA conv (its leaky_relu'd input and its weight) to bf16 first, as the bf16 kernels do, keeping the rest in the
working dtype.  random_state_dict() builds a checkpoint whose convs have roughly unit gain.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from kokoro_ruslan_amd.vocoder import layer_shapes, resolve_config


def _r(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def forward(weights: Dict[str, torch.Tensor], biases: Dict[str, torch.Tensor], config: Optional[dict], mel: torch.Tensor,
            round_bf16: bool = False) -> torch.Tensor:
    cfg = resolve_config(config)
    dt = weights["conv_pre"].dtype
    W = lambda n: _r(weights[n], round_bf16)
    single = mel.dim() == 2
    x = (mel[None] if single else mel).to(dt).transpose(1, 2)                       # [B, 80, T]
    x = F.conv1d(_r(x, round_bf16), W("conv_pre"), biases["conv_pre"].to(dt), padding=3)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(_r(x, round_bf16), W(f"ups.{i}"), biases[f"ups.{i}"].to(dt), stride=u, padding=(k - u) // 2)
        xs = None
        for j, (rk, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            h = x
            for m, d in enumerate(ds):
                n = f"resblocks.{i * nk + j}"
                t = F.conv1d(_r(F.leaky_relu(h, 0.1), round_bf16), W(f"{n}.convs1.{m}"), biases[f"{n}.convs1.{m}"].to(dt),
                             dilation=d, padding=(rk * d - d) // 2)
                t = F.conv1d(_r(F.leaky_relu(t, 0.1), round_bf16), W(f"{n}.convs2.{m}"), biases[f"{n}.convs2.{m}"].to(dt),
                             padding=(rk - 1) // 2)
                h = t + h
            xs = h if xs is None else xs + h
        x = xs / nk
    x = F.leaky_relu(x)                                                             # default slope 0.01
    x = F.conv1d(x, weights["conv_post"], biases["conv_post"].to(dt), padding=3)     # fp32 in both math modes
    y = torch.tanh(x)[:, 0]
    return y[0] if single else y


def random_state_dict(config: Optional[dict] = None, seed: int = 0, form: str = "weight_norm") -> Dict[str, torch.Tensor]:
    """A generator state dict with v ~ N(0, 1) and g picked so that each conv has roughly unit gain (the reference's N(0, 0.01) init
    drives the waveform to ~0).  form: "weight_norm" (weight_g / weight_v), "parametrizations" (original0 / original1) or "plain"."""
    cfg = resolve_config(config)
    gen = torch.Generator().manual_seed(seed)
    rates = dict((f"ups.{i}", int(u)) for i, u in enumerate(cfg["upsample_rates"]))
    sd = {}
    for name, (kind, shape) in layer_shapes(cfg).items():
        v = torch.randn(*shape, generator=gen)
        if kind == "convt":          # dim 0 = Cin: a unit-norm row of Cin feeds cout * k / stride outputs per input position
            cin, cout, _ = shape
            gain = math.sqrt(cout * rates[name] / cin)
        else:
            gain = 1.0
        g = torch.full((shape[0], 1, 1), gain) * (1.0 + 0.1 * torch.rand(shape[0], 1, 1, generator=gen))
        b = 0.1 * torch.randn(shape[1] if kind == "convt" else shape[0], generator=gen)
        if form == "weight_norm":
            sd[f"{name}.weight_g"], sd[f"{name}.weight_v"] = g, v
        elif form == "parametrizations":
            sd[f"{name}.parametrizations.weight.original0"], sd[f"{name}.parametrizations.weight.original1"] = g, v
        elif form == "plain":
            sd[f"{name}.weight"] = v * (g / v.norm(2, dim=(1, 2), keepdim=True))
        else:
            raise ValueError(form)
        sd[f"{name}.bias"] = b
    return sd
