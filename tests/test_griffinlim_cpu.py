"""Griffin-Lim without a GPU: the restated mel filterbank and its inversion, the torch restatement's fp32 drift against fp64, the
reference's random phase draws, argument checks, and the kokoro-synth --griffin-lim flags."""
import pytest
import torch

from kokoro_ruslan_amd import griffinlim_torch as GT
from kokoro_ruslan_amd.griffinlim import (GriffinLimVocoder, check_args, inverse_mel_matrix, melscale_fbanks, random_angles,
                                          twiddles)


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def test_filterbank_shape_rank_and_support():
    fb = melscale_fbanks(torch.float64)
    assert fb.shape == (513, 80)
    assert int(torch.linalg.matrix_rank(fb)) == 80
    live = (fb.sum(1) > 0).nonzero().flatten()
    assert live[0].item() == 1 and live[-1].item() == 371 and live.numel() == 371
    assert 5.5 < float(torch.linalg.cond(fb.t())) < 6.5
    # a triangle peaks at 1 at its centre (norm=None) and the HTK end points are 0 and 8000 Hz
    assert float(fb.max()) <= 1.0 and float(fb.max()) > 0.9


def test_pinv_matches_gels_least_squares():
    mel = GT.harmonic_logmel(120, seed=3)
    E = torch.exp(mel.float()).t()
    fbt = melscale_fbanks(torch.float64).t().float()
    gels = torch.relu(torch.linalg.lstsq(fbt[None], E[None], driver="gels").solution[0])
    pinv = torch.relu(inverse_mel_matrix().float() @ E)
    assert _rel(pinv, gels.double()) <= 1e-5, _rel(pinv, gels.double())
    # S = P^(1/2) magnifies the fp32 rounding of P ~ 0 (bin 0, bins above 371): the reference's own fp32 S is ~1e-4 from fp64's
    assert _rel(GT.magnitude(mel.float(), torch.float32, solver="gels"), GT.magnitude(mel)) <= 3e-4


@pytest.mark.parametrize("n_iter,bound", [(1, 2e-6), (4, 6e-6), (16, 2e-4), (60, 1e-2)])
def test_restatement_fp32_tracks_fp64(n_iter, bound):
    mel = GT.harmonic_logmel(300)
    S = GT.magnitude(mel)
    ang = torch.rand((513, 300), dtype=torch.complex64, generator=torch.Generator().manual_seed(0))
    y64 = GT.griffinlim(S, ang, n_iter)
    y32 = GT.griffinlim(S.float(), ang, n_iter)
    assert y64.shape == (256 * 299,)
    assert _rel(y32, y64) <= bound, (n_iter, _rel(y32, y64))
    assert abs(GT.spectral_convergence(y32, S) - GT.spectral_convergence(y64, S)) <= 1e-4


def test_spectral_convergence_falls_with_iterations():
    mel = GT.harmonic_logmel(200, seed=1)
    S = GT.magnitude(mel)
    ang = torch.rand((513, 200), dtype=torch.complex64, generator=torch.Generator().manual_seed(1))
    sc = [GT.spectral_convergence(GT.griffinlim(S, ang, n), S) for n in (0, 4, 30)]
    assert sc[0] > sc[1] > sc[2]


def test_random_angles_follow_the_reference_draw_order():
    frames = [7, 300, 4]
    g = torch.Generator().manual_seed(42)
    got = random_angles(frames, torch.Generator().manual_seed(42))
    for f, a in zip(frames, got):
        want = torch.rand((1, 513, f), dtype=torch.complex64, generator=g)
        assert a.shape == (513, f) and torch.equal(a, want[0])
        assert 0 <= float(a.real.min()) and float(a.real.max()) < 1 and 0 <= float(a.imag.min()) and float(a.imag.max()) < 1
    torch.manual_seed(5)
    glob = random_angles(frames)
    torch.manual_seed(5)
    assert all(torch.equal(a, torch.rand((1, 513, f), dtype=torch.complex64)[0]) for a, f in zip(glob, frames))


def test_twiddle_table_is_fp64_rounded():
    tw = twiddles()
    j = torch.arange(1024, dtype=torch.float64)
    want = torch.complex(torch.cos(2 * torch.pi * j / 1024), -torch.sin(2 * torch.pi * j / 1024)).to(torch.complex64)
    assert torch.equal(tw, want)


def test_argument_checks():
    check_args(0, 0.0, "ones")
    for bad in ((-1, 0.99, "random"), (60, 1.0, "random"), (60, -0.1, "random"), (60, 0.99, "zeros"), (2.5, 0.99, "random")):
        with pytest.raises(ValueError):
            check_args(*bad)
    voc = GriffinLimVocoder(device="cpu")                      # the checks run before anything touches the device
    with pytest.raises(ValueError, match="at least 4"):
        voc.vocode([torch.zeros(10, 80), torch.zeros(3, 80)])
    with pytest.raises(ValueError, match="expected"):
        voc.vocode([torch.zeros(10, 64)])
    with pytest.raises(ValueError, match="expected"):
        voc.vocode([torch.zeros(80)])
    with pytest.raises(ValueError, match="momentum"):
        voc.vocode([torch.zeros(10, 80)], momentum=1.5)
    with pytest.raises(ValueError, match="n_iter"):
        voc.vocode([torch.zeros(10, 80)], n_iter=-2)
    with pytest.raises(ValueError, match="angles 0"):
        voc.vocode([torch.zeros(10, 80)], angles=[torch.zeros(513, 9, dtype=torch.complex64)])
    assert voc.sampling_rate == 22050 and voc.hop == 256


def test_tile_table_covers_each_utterance():
    voc = GriffinLimVocoder(device="cpu")
    frames = [4, 8, 9, 17]
    t = voc.tiles(frames)
    F = voc.tile_frames
    assert t.dtype == torch.int32 and t.shape == (sum((f + F - 1) // F for f in frames), 4)
    start, wav = 0, 0
    for f in frames:
        rows = t[t[:, 0] == start]
        assert rows[:, 1].eq(f).all() and rows[:, 2].tolist() == list(range(0, f, F)) and rows[:, 3].eq(wav).all()
        start, wav = start + f, wav + 256 * (f - 1)


def test_cli_griffin_lim_flags():
    from kokoro.cli import synth as cli
    base = ["--checkpoint", "c", "--ids", "u.jsonl", "--output", "o"]
    p = cli.build_parser()
    a = p.parse_args(base + ["--griffin-lim", "--griffin-lim-iters", "12", "--griffin-lim-seed", "3"])
    cli.check_args(p, a)
    assert a.griffin_lim and a.griffin_lim_iters == 12 and a.griffin_lim_seed == 3
    a = p.parse_args(base)
    cli.check_args(p, a)
    assert not a.griffin_lim and a.griffin_lim_iters == 60 and a.griffin_lim_seed is None and a.vocoder is None
    for bad in (["--griffin-lim", "--vocoder", "hifigan"], ["--griffin-lim-iters", "5"], ["--griffin-lim-seed", "1"],
                ["--griffin-lim", "--griffin-lim-iters", "-1"]):
        with pytest.raises(SystemExit):
            cli.check_args(p, p.parse_args(base + bad))
    with pytest.raises(SystemExit):                           # the conflict is refused before any checkpoint is read
        cli.main(base + ["--griffin-lim", "--vocoder", "hifigan"])
