"""GPU suite, kernel level: kk_prosody_durations and kk_prosody_variance through kk.call against their fp32 torch restatement
(kokoro_ruslan_amd/prosody_torch.py, run on the host) with torch.equal.  Shapes straddle a wave (64) and a workgroup (256)."""
import math

import pytest
import torch

from kokoro_ruslan_amd import prosody_torch as PT

pytestmark = pytest.mark.gpu

B = 3
JUST_BELOW_HALF = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))      # the fp32 neighbour


def _kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib as kk
    return kk


def _row_lengths(Pn):
    return [max(1, n) for n in (1, Pn - 1, Pn)]


def _duration_inputs(Pn, seed):
    """d, speed, forced with the edge cases at fixed places (as far as Pn has room): d / speed exactly k + 0.5, d just below 0.5, d
    exactly 0.5 and 1.5 (half to even at speed 1), a negative d, a scaled value below one frame, forced 0 / > 0 over both kinds of d."""
    g = torch.Generator().manual_seed(seed)
    d = (torch.randn(B, Pn, generator=g) * 4 + 3).float()
    speed = (0.25 + 3.75 * torch.rand(B, Pn, generator=g)).float()
    forced = torch.where(torch.rand(B, Pn, generator=g) < 0.25, torch.randint(0, 9, (B, Pn), generator=g), torch.tensor(-1)).to(torch.int32)
    edge = [(5.0, 2.0, -1),                                    # 2.5 exactly -> 2
            (7.0, 2.0, -1),                                    # 3.5 exactly -> 4
            (0.75, 0.5, -1),                                   # 1.5 exactly -> 2
            (JUST_BELOW_HALF, 1.0, -1),                        # just under a half: base 0
            (0.5, 1.0, -1), (1.5, 1.0, -1),                    # half to even at speed 1: 0 and 2
            (-2.0, 1.0, -1), (1.0, 4.0, -1),                   # negative -> 0; 0.25 frames -> 1, the phoneme is kept
            (0.2, 1.0, 5), (6.0, 2.0, 0)]                      # forced over a zero and a zero forced over frames
    for b in range(B):
        for k, (dv, sv, fv) in enumerate(edge if Pn >= len(edge) else [edge[3 * b]]):     # (Pn = 1: one edge case per row)
            p = (k + b) % Pn
            d[b, p], speed[b, p], forced[b, p] = dv, sv, fv
    return d, speed, forced


@pytest.mark.parametrize("with_plens", [False, True], ids=["plens-null", "plens"])
@pytest.mark.parametrize("Pn", [1, 64, 65, 300])
def test_prosody_durations_equals_the_restatement(Pn, with_plens):
    kk = _kk()
    d, speed, forced = _duration_inputs(Pn, 11 + Pn)
    if Pn >= 64:
        q = d / speed
        assert bool(((q - q.floor()) == 0.5).any()) and bool(((d < 0.5) & (d > 0.4999999)).any()), "the inputs hold the edge cases"
    plens = torch.tensor(_row_lengths(Pn), dtype=torch.int32) if with_plens else None
    want, want_sums = PT.durations(d, speed, forced, plens)
    dur = torch.full((B, Pn), -7, dtype=torch.int64, device="cuda")
    sums = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    kk.call("kk_prosody_durations", d.cuda(), speed.cuda(), forced.cuda(), plens.cuda() if with_plens else None, dur, sums, B, Pn)
    assert torch.equal(dur.cpu(), want) and torch.equal(sums.cpu(), want_sums)
    if with_plens:
        for b, n in enumerate(_row_lengths(Pn)):
            assert int(dur[b, n:].abs().sum()) == 0
    # neutral tables: clamp(round(d), 0), bit for bit
    one, none = torch.ones(B, Pn, device="cuda"), torch.full((B, Pn), -1, dtype=torch.int32, device="cuda")
    kk.call("kk_prosody_durations", d.cuda(), one, none, None, dur, sums, B, Pn)
    ref = torch.clamp(torch.round(d), min=0).to(torch.int64)
    assert torch.equal(dur.cpu(), ref) and torch.equal(sums.cpu(), ref.sum(dim=1))


def _variance_inputs(Pn, T, seed):
    g = torch.Generator().manual_seed(seed)
    pitch = (torch.randn(B, T, generator=g) * 0.6 + 0.4).float()
    energy = (torch.randn(B, T, generator=g) * 0.6 + 0.5).float()
    for b in range(B):                                              # exact 0 and 1, and values the clamp brings there
        for k, v in enumerate((0.0, 1.0, -0.0, 1.5, -0.5) if T >= 8 else (0.0, 1.0, -0.5)):
            pitch[b, (k + b) % T] = v
            energy[b, (k + 2 * b + 1) % T] = v
    lens = torch.tensor([max(1, n) for n in (1, T - 1, T)], dtype=torch.int64)
    idx = torch.sort(torch.randint(0, Pn, (B, T), generator=g), dim=1).values          # frames of a phoneme are contiguous
    idx = torch.where(torch.arange(T)[None, :] < lens[:, None], idx, torch.tensor(-1))  # what kk_length_regulate_index writes
    ps, es = 2.0 * torch.rand(B, Pn, generator=g), 2.0 * torch.rand(B, Pn, generator=g)
    pb, eb = torch.rand(B, Pn, generator=g) - 0.5, torch.rand(B, Pn, generator=g) - 0.5
    nan = torch.tensor(math.nan)
    fp = torch.where(torch.rand(B, Pn, generator=g) < 0.3, torch.rand(B, Pn, generator=g), nan)
    fe = torch.where(torch.rand(B, Pn, generator=g) < 0.3, torch.rand(B, Pn, generator=g), nan)
    if Pn > 1:                                                      # both kinds of entries in every table, whatever the draw
        fp[:, 0], fe[:, 0], fp[:, 1], fe[:, 1] = math.nan, 0.0, 1.0, math.nan
    return pitch, energy, idx, lens, ps, pb, es, eb, fp, fe


@pytest.mark.parametrize("Pn,T", [(1, 3), (64, 256), (65, 257), (300, 700), (64, 700), (300, 3)])
def test_prosody_variance_equals_the_restatement(Pn, T):
    kk = _kk()
    args = _variance_inputs(Pn, T, 5 + Pn + T)
    pitch, fp = args[0], args[8]
    assert bool((pitch == 0).any()) and bool((pitch == 1).any())
    if Pn > 1:
        assert bool(torch.isnan(fp).any()) and bool((~torch.isnan(fp)).any())
    want_p, want_e = PT.variance(*args)
    out_p, out_e = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7.0, device="cuda")
    kk.call("kk_prosody_variance", *[a.cuda().contiguous() for a in args], out_p, out_e, B, Pn, T)
    assert torch.equal(out_p.cpu(), want_p) and torch.equal(out_e.cpu(), want_e)
    lens = args[3]
    for b in range(B):                                              # frames past the row's length: the clamped prediction
        n = int(lens[b])
        assert torch.equal(out_p[b, n:].cpu(), pitch[b, n:].clamp(0, 1))
    # neutral tables: the clamp, bit for bit
    one, zero, nan = (torch.full((B, Pn), v, device="cuda") for v in (1.0, 0.0, math.nan))
    kk.call("kk_prosody_variance", args[0].cuda(), args[1].cuda(), args[2].cuda(), lens.cuda(), one, zero, one, zero, nan, nan, out_p, out_e, B, Pn, T)
    assert torch.equal(out_p.cpu(), args[0].clamp(0, 1)) and torch.equal(out_e.cpu(), args[1].clamp(0, 1))
