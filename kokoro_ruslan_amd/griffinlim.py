"""Griffin-Lim vocoding on the device: a batch of log-mels [frames_b, 80] to waveforms, on the kernels of csrc/kk_griffinlim.hip.

`GriffinLimVocoder` restates the reference's second vocoder, torchaudio's InverseMelScale + GriffinLim with hard-coded settings:
22050 Hz, n_fft = win = 1024, hop = 256, 80 HTK mels over 0-8000 Hz without norm, power 2, periodic Hann, center with reflect
padding.  The mel inversion's least-squares solution is the minimum-norm one, pinv(fb^T) . exp(mel) (fb^T has full row rank), with
pinv computed once in fp64.  The mels of one call are packed back to back along frames and run through one init launch, one fused
launch per iteration and one final iSTFT launch; each utterance's sums run in an order fixed by its own frames, so row b of a batch is,
bit for bit, the utterance vocoded alone.  All arithmetic is fp32, as in the reference.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from kokoro_ruslan_amd import lib as kk
from kokoro_ruslan_amd.stft import HOP, N_BINS, N_FFT, N_MELS, SAMPLE_RATE, device_tables
from kokoro_ruslan_amd.stft import hann_window, twiddles  # noqa: F401  (re-exported: tests and tools import them from here)

F_MAX = 8000.0
MIN_FRAMES = 4                          # the STFT's reflect padding (512) needs a signal of 256 (T - 1) > 512 samples
DEFAULT_MAX_FRAMES = 1 << 18            # packed frames per group (S, rebuilt and two spectra: 7 x 513 floats per frame, ~3.8 GB)


def melscale_fbanks(dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """torchaudio.functional.melscale_fbanks(513, 0, 8000, 80, 22050, norm=None, mel_scale="htk"): [513, 80] triangles."""
    all_freqs = torch.linspace(0, SAMPLE_RATE // 2, N_BINS, dtype=dtype)
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    m_pts = torch.linspace(mel(0.0), mel(F_MAX), N_MELS + 2, dtype=dtype)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0)


def inverse_mel_matrix() -> torch.Tensor:
    """pinv(fb^T) [513, 80] in fp64: P = relu(pinv(fb^T) . exp(mel)) is InverseMelScale's gels solution (fb^T has full row rank)."""
    return torch.linalg.pinv(melscale_fbanks(torch.float64).t())


def check_args(n_iter: int, momentum: float, init: str) -> None:
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError(f"n_iter must be an integer >= 0, not {n_iter!r}")
    if not 0 <= momentum < 1:
        raise ValueError(f"momentum must be in [0, 1), not {momentum!r} (as torchaudio's GriffinLim)")
    if init not in ("random", "ones"):
        raise ValueError(f"init must be 'random' or 'ones', not {init!r}")


def check_mel(i: int, m: torch.Tensor) -> None:
    if m.dim() != 2 or m.shape[1] != N_MELS:
        raise ValueError(f"mel {i}: shape {tuple(m.shape)}, expected [frames, {N_MELS}]")
    if m.shape[0] < MIN_FRAMES:
        raise ValueError(f"mel {i}: {m.shape[0]} frames; Griffin-Lim needs at least {MIN_FRAMES}: the STFT reflect-pads "
                         f"{N_FFT // 2} samples at each end of a signal of {HOP} (frames - 1) samples, which must be longer")


def random_angles(frames: Sequence[int], generator: Optional[torch.Generator] = None) -> List[torch.Tensor]:
    """The reference's rand_init phases, one utterance at a time in input order: torch.rand((1, 513, T), complex64) on the CPU
    (real and imaginary parts uniform on [0, 1)).  Returned as [513, T]."""
    return [torch.rand((1, N_BINS, int(t)), dtype=torch.complex64, generator=generator)[0] for t in frames]


class GriffinLimVocoder:
    """Batched Griffin-Lim on the MI355X: vocode(list of [frames_b, 80] log-mels) -> waveforms of 256 (frames_b - 1) samples."""

    sampling_rate = SAMPLE_RATE
    hop = HOP

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        self.pinv = inverse_mel_matrix().to(torch.float32).contiguous().to(self.device)
        self.window, self.tw = device_tables(self.device)
        self.tile_frames = int(kk.load().kk_gl_tile_frames())
        self._ws: Optional[torch.Tensor] = None

    def _workspace(self, floats: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < floats:
            self._ws = None
            self._ws = torch.empty(floats, dtype=torch.float32, device=self.device)
        return self._ws

    def tiles(self, frames: Sequence[int]) -> torch.Tensor:
        """int32 [ntiles, 4]: {utterance start frame, frames, first frame of the tile, first sample in the packed waveform}."""
        rows, start, wav = [], 0, 0
        for t in frames:
            rows += [[start, t, f0, wav] for f0 in range(0, t, self.tile_frames)]
            start += t
            wav += HOP * (t - 1)
        return torch.tensor(rows, dtype=torch.int32)

    def vocode(self, mels: Sequence[torch.Tensor], n_iter: int = 60, momentum: float = 0.99, init: str = "random",
               generator: Optional[torch.Generator] = None, angles: Optional[Sequence[torch.Tensor]] = None,
               max_frames: int = DEFAULT_MAX_FRAMES) -> List[torch.Tensor]:
        """One fp32 waveform of 256 (frames_b - 1) samples per log-mel [frames_b, 80], in input order.  init "random" draws the
        reference's phases (random_angles, with `generator`), "ones" starts from phase 0; angles= gives the initial phases [513,
        frames_b] (complex) of every mel explicitly.  The mels run in groups of at most max_frames packed frames (a longer mel runs
        alone)."""
        check_args(n_iter, momentum, init)
        for i, m in enumerate(mels):
            check_mel(i, m)
        frames = [int(m.shape[0]) for m in mels]
        if angles is not None:
            angles = list(angles)
            if len(angles) != len(mels):
                raise ValueError(f"{len(angles)} angle tensors for {len(mels)} mels")
            for i, (a, t) in enumerate(zip(angles, frames)):
                if tuple(a.shape[-2:]) != (N_BINS, t) or a.dim() not in (2, 3) or (a.dim() == 3 and a.shape[0] != 1):
                    raise ValueError(f"angles {i}: shape {tuple(a.shape)}, expected [{N_BINS}, {t}]")
            angles = [a.reshape(N_BINS, t) for a, t in zip(angles, frames)]
        elif init == "random":
            angles = random_angles(frames, generator)
        beta = momentum / (1 + momentum) if momentum else 0.0
        out: List[torch.Tensor] = []
        group, total = [], 0
        for i, t in enumerate(frames):
            if group and total + t > max_frames:
                out += self._run([mels[j] for j in group], [angles[j] for j in group] if angles is not None else None, n_iter, beta)
                group, total = [], 0
            group.append(i)
            total += t
        if group:
            out += self._run([mels[j] for j in group], [angles[j] for j in group] if angles is not None else None, n_iter, beta)
        return out

    def _run(self, mels: List[torch.Tensor], angles: Optional[List[torch.Tensor]], n_iter: int, beta: float) -> List[torch.Tensor]:
        dev = self.device
        frames = [int(m.shape[0]) for m in mels]
        T = sum(frames)
        x = torch.cat([m.to(dev, torch.float32) for m in mels]).contiguous()
        ang = None
        if angles is not None:
            ang = torch.view_as_real(torch.cat([a.to(torch.complex64).t() for a in angles]).contiguous()).to(dev)
        tiles = self.tiles(frames).to(dev)
        nt = tiles.shape[0]
        n = T * N_BINS
        ws = self._workspace(7 * n)
        S, Ya, Yb, R = ws[:n], ws[n:3 * n], ws[3 * n:5 * n], ws[5 * n:7 * n]
        kk.call("kk_gl_init", x, T, self.pinv, ang, S, Ya, R)
        for _ in range(n_iter):
            kk.call("kk_gl_iter", Ya, Yb, R, S, tiles, nt, self.tw, self.window, beta)
            Ya, Yb = Yb, Ya
        wave = torch.empty(HOP * (T - len(frames)), dtype=torch.float32, device=dev)
        kk.call("kk_gl_istft", Ya, tiles, nt, self.tw, self.window, wave)
        return list(wave.split([HOP * (f - 1) for f in frames]))
