"""The inputs the long-form tests share (test_longform_cpu.py, test_longform_kernels_gpu.py): a table of mels that walks every branch
of the trailing-silence trim, and the chunk lengths, gaps and documents of the join.  Built from fixed seeds; nothing here calls the
code under test.

A mel is made from a profile of frame means: frame t is its mean m_t plus noise in [-0.4, 0.4] whose own mean over the channels is
removed in fp64, so the frame mean of the fp32 mel is m_t to a few ulps and every decision margin is known by construction:
  voiced frames    m_t in [-6, -3]
  silent frames    m_t in [-10.95, -10.65] (all values above the clamp's floor of -11.5)
  cluster A / B    m_t within 0.02 of -9.7 / -9.3: with 15 % of the frames in each, q10 falls into A and q20 into B, so the
                   unclipped threshold is near -9.5, strictly inside [-9.8, -9.2], and B is voiced while A is not
The threshold is -9.8 ("under") when more than 20 % of the frames are silent, -9.2 ("over") when none is."""
import math

import torch

N_MELS = 80
T_REQUIRED = (1, 2, 59, 60, 61, 64, 65, 257, 1024, 4096)


def _mel(means: torch.Tensor, g: torch.Generator, n_mels: int) -> torch.Tensor:
    noise = 0.8 * (torch.rand(means.numel(), n_mels, generator=g, dtype=torch.float64) - 0.5)
    noise -= noise.mean(dim=1, keepdim=True)
    return (means.to(torch.float64)[:, None] + noise).to(torch.float32)


def _voiced(n, g):
    return -6.0 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)


def _silent(n, g):
    return -10.95 + 0.3 * torch.rand(n, generator=g, dtype=torch.float64)


def _cluster(n, centre, g):
    return centre + 0.04 * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5)


def _lead(T, voiced, g):
    """`voiced` voiced frames, then silence to T."""
    return torch.cat([_voiced(voiced, g), _silent(T - voiced, g)])


def _inside(T, g):
    """voiced frames, then 15 % of the frames in cluster A and 15 % in cluster B, shuffled, at the tail."""
    n = int(math.ceil(0.15 * T))
    tail = torch.cat([_cluster(n, -9.7, g), _cluster(n, -9.3, g)])
    return torch.cat([_voiced(T - 2 * n, g), tail[torch.randperm(2 * n, generator=g)]])


def finish_cases(n_mels: int = N_MELS):
    """[(name, mel fp32 [T, n_mels], the threshold branch the case is there for: "under" | "over" | "inside" | "nan")]"""
    g = torch.Generator().manual_seed(20240611)
    table = []

    def add(name, means, branch, edit=None):
        mel = _mel(means, g, n_mels)
        if edit is not None:
            edit(mel)
        table.append((name, mel, branch))

    add("T1-over", _voiced(1, g), "over")
    add("T2-under-unvoiced", _silent(2, g), "under")
    add("T59-over-all-voiced", _voiced(59, g), "over")
    add("T60-under-keeps-60", _lead(60, 10, g), "under")                  # proposed_end 34 < 60 = T
    add("T61-under-keeps-60", _lead(61, 5, g), "under")                   # proposed_end 29 < 60 < T
    add("T64-inside", _inside(64, g), "inside")
    add("T65-under-near-end", _lead(65, 51, g), "under")                  # last voiced 50: 14 frames from the end
    add("T257-under-far", _lead(257, 151, g), "under")                    # t_end 175

    def extremes(mel):                                                    # values outside [-11.5, 2]: the clamp moves the frame means
        mel[0:151:3, 5] = 5.0
        mel[151::2, 7] = -20.7
        mel[200, :] = -20.7
        mel[3, 1] = 2.0
        mel[4, 2] = -11.5
    add("T257-outside-clamp", _lead(257, 151, g), "under", extremes)
    add("T1024-inside", _inside(1024, g), "inside")
    add("T4096-under-far", _lead(4096, 3001, g), "under")
    add("T4096-over", _voiced(4096, g), "over")

    def one_nan(mel):
        mel[17, 3] = float("nan")
    add("T300-nan", _lead(300, 120, g), "nan", one_nan)
    return table


CHUNK_LENGTHS = (1, 255, 256, 257, 3307, 5000)
GAPS = (0, 1, 3307)
DOCUMENTS = ([2], [0, 4, 1], [5], [3])         # documents of 1 and 3 chunks, not in chunk order


def join_chunks_input():
    g = torch.Generator().manual_seed(77)
    return [torch.rand(n, generator=g) * 2.0 - 1.0 for n in CHUNK_LENGTHS]


def cat_documents(chunks, documents, gap):
    """The reference's construction (inference.py:643-648): torch.cat of the chunks with torch.zeros(gap) between them."""
    out = []
    for d in documents:
        parts = []
        for k, c in enumerate(d):
            if k:
                parts.append(torch.zeros(gap, dtype=chunks[c].dtype, device=chunks[c].device))
            parts.append(chunks[c])
        out.append(torch.cat(parts))
    return out
