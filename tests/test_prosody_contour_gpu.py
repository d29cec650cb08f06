"""GPU suite: frame-level prosody contours.  kk_prosody_contour through kk.call against its fp32 torch restatement
(prosody_torch.contour, run on the host) with torch.equal at the scan's wave (64) and workgroup (256) edges; the engine's three
entry points with a contour per row; kokoro-eval --oracle-prosody on a temporary cache.

The engine comparisons are exact and need no margins: the oracle is given the engine's own predictions (syn.out.pitch /
syn.out.energy), so both sides bucketize the same fp32 values."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prosody_contour_cases as CC  # noqa: E402
import test_prosody_gpu as TP  # noqa: E402  (the tiny model and the utterances of the prosody engine tests)
from kokoro_ruslan_amd import prosody_torch as PT  # noqa: E402
from kokoro_ruslan_amd.prosody import Prosody, pack, pack_contours  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = math.nan
VA = TP.VA
KW = TP.KW
SIZES = TP.SIZES


def _kk():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import lib as kk
    return kk


def _equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _run(kk, args, rows=None):
    """kk_prosody_contour on the rows `rows` (default: all) of the host inputs `args`; returns the two outputs on the host."""
    rows = list(range(args[0].shape[0])) if rows is None else rows
    dev = [None if a is None else a[rows].contiguous().cuda() for a in args]
    B, T = dev[0].shape
    Pn, Sn = dev[4].shape[1], next((a.shape[1] for a in dev[12:] if a is not None), 0)
    out_p, out_e = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7.0, device="cuda")
    kk.call("kk_prosody_contour", *dev, out_p, out_e, B, Pn, T, Sn)
    return out_p.cpu(), out_e.cpu()


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    """Pn -> (inputs, the oracle's outputs): computed once."""
    out = {}
    for Pn in (1, 63, 64, 65, 257, 1025):
        args = CC.kernel_inputs(Pn, 100 + Pn)
        out[Pn] = (args, PT.contour(*args))
    return out


@pytest.mark.parametrize("Pn", [1, 63, 64, 65, 257, 1025])
def test_contour_kernel_equals_the_restatement(cases, Pn):
    kk = _kk()
    args, (want_p, want_e) = cases[Pn]
    dur, sd, pc, ec, lens, T = args[10], args[11], args[12], args[13], args[3], args[0].shape[1]
    assert T % 64 != 0 and len(set(lens.tolist())) == 3, "ragged rows, no whole number of waves"
    assert int(sd[0].sum()) == 0 and bool(torch.isnan(ec[1]).all()) and bool(torch.isnan(pc[0]).all())
    if Pn >= 63:
        assert bool(((dur[2] == 0) & (sd[2] > 0)).any()) and bool(((dur[2] > 0) & (sd[2] == 0)).any())
        assert bool(torch.isnan(pc[2, :int(sd[2].sum())]).any()) and bool((pc[1] == 0).any())
    got_p, got_e = _run(kk, args)
    assert _equal(got_p, want_p) and _equal(got_e, want_e)
    v_p, v_e = PT.variance(*args[:10])
    assert torch.equal(got_p[0], v_p[0]) and torch.equal(got_e[0], v_e[0]) and torch.equal(got_e[1], v_e[1]), "no track: today's values"
    if Pn >= 63:
        assert not torch.equal(got_p[1], v_p[1]) and not torch.equal(got_e[2], v_e[2]), "the contours act"


def test_contour_kernel_takes_a_null_track(cases):
    kk = _kk()
    args, (want_p, want_e) = cases[65]
    v_p, v_e = PT.variance(*args[:10])
    got_p, got_e = _run(kk, args[:13] + (None,))
    assert _equal(got_p, want_p) and torch.equal(got_e, v_e)
    got_p, got_e = _run(kk, args[:12] + (None, args[13]))
    assert torch.equal(got_p, v_p) and _equal(got_e, want_e)


@pytest.mark.parametrize("Pn", [65, 257])
def test_contour_kernel_rows_alone_and_in_another_order(cases, Pn):
    kk = _kk()
    args, _ = cases[Pn]
    got_p, got_e = _run(kk, args)
    for b in range(3):
        one_p, one_e = _run(kk, args, [b])
        assert _equal(one_p[0], got_p[b]) and _equal(one_e[0], got_e[b]), f"row {b} alone"
    perm = [2, 0, 1]
    per_p, per_e = _run(kk, args, perm)
    for k, b in enumerate(perm):
        assert _equal(per_p[k], got_p[b]) and _equal(per_e[k], got_e[b]), f"row {b} at place {k}"


@pytest.mark.parametrize("Pn", [1, 64, 257])
def test_contour_kernel_with_nan_tracks_equals_the_variance_kernel(cases, Pn):
    kk = _kk()
    args, _ = cases[Pn]
    nan = torch.full_like(args[12], NAN)
    got_p, got_e = _run(kk, args[:12] + (nan, nan))
    dev = [a.contiguous().cuda() for a in args[:10]]
    B, T = dev[0].shape
    ref_p, ref_e = torch.full((B, T), -7.0, device="cuda"), torch.full((B, T), -7.0, device="cuda")
    kk.call("kk_prosody_variance", *dev, ref_p, ref_e, B, Pn, T)
    assert torch.equal(got_p, ref_p.cpu()) and torch.equal(got_e, ref_e.cpu())


def test_beyond_the_limits_python_raises_before_any_launch():
    kk = _kk()
    before = kk.launches
    with pytest.raises(ValueError, match="4097 phonemes"):
        pack_contours([Prosody(pitch_contour=[0.5], contour_durations=[1] + [0] * 4096)], [4097], 4097, "cuda")
    with pytest.raises(ValueError, match="4096"):
        pack_contours([Prosody(pitch_contour=[0.5] * 4097, contour_durations=[4097])], [1], 1, "cuda")
    with pytest.raises(ValueError, match="4096"):
        Prosody.from_tracks([4097], [0.5] * 4097).validate(1)
    assert kk.launches == before


# ---- 2. the engine ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d, P = TP.fixture_model()
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    ids, st = TP.utterances(d)
    return d, e, [u.cuda() for u in ids], [s.cuda() for s in st]


def _launch_names(monkeypatch, fn):
    from kokoro_ruslan_amd import lib as kk
    names, real = [], kk.call
    with monkeypatch.context() as m:
        m.setattr(kk, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        out = fn()
    return names, out


def _per_phoneme(n, seed):
    g = torch.Generator().manual_seed(seed)
    pv, ev = (0.05 + 0.9 * torch.rand(n, generator=g)), (0.05 + 0.9 * torch.rand(n, generator=g))
    pv[n // 2] = 0.0                                               # an unvoiced phoneme
    return pv, ev


def test_a_contour_constant_over_each_phoneme_equals_the_forced_values(world, monkeypatch):
    d, e, ids, st = world
    forced, contour = [], []
    for k, n in enumerate(SIZES):
        pv, ev = _per_phoneme(n, 20 + k)
        cd = 1 + torch.arange(n) % 3                               # any source length >= 1: the value is the same all over
        forced.append(Prosody(pitch=pv, energy=ev))
        contour.append(Prosody(pitch_contour=pv.repeat_interleave(cd), energy_contour=ev.repeat_interleave(cd), contour_durations=cd))
    names_f, (a, ia) = _launch_names(monkeypatch, lambda: e.generate_batch(ids, st, want_info=True, prosody=forced, **KW))
    names_c, (b, ib) = _launch_names(monkeypatch, lambda: e.generate_batch(ids, st, want_info=True, prosody=contour, **KW))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and ia["T"] == ib["T"] and ia["bounds"] == ib["bounds"]
    assert "kk_prosody_contour" not in names_f and names_f.count("kk_prosody_variance") == 1
    assert "kk_prosody_variance" not in names_c and names_c.count("kk_prosody_contour") == 1
    assert [n for n in names_c if n != "kk_prosody_contour"] == [n for n in names_f if n != "kk_prosody_variance"]
    names_0, _ = _launch_names(monkeypatch, lambda: e.generate_batch(ids, st, **KW))
    assert not any(n.startswith("kk_prosody") for n in names_0), "prosody=None: the launches are today's"
    pad = torch.zeros(1, SIZES[1], dtype=torch.int64, device="cuda")
    pad[0] = ids[1]
    names_g, _ = _launch_names(monkeypatch, lambda: e.generate(pad, None, prosody=forced[1], **KW))
    names_s, _ = _launch_names(monkeypatch, lambda: e.generate_stream(ids, st, slots=2, prosody=forced, **KW))
    assert "kk_prosody_contour" not in names_g + names_s and "kk_prosody_variance" in names_g and "kk_prosody_variance" in names_s


def _varying(n, dur, seed):
    """A contour over the model's own durations `dur` that moves inside every phoneme: source frames 2 per frame."""
    g = torch.Generator().manual_seed(seed)
    cd = 2 * dur.cpu().clamp(min=1)
    S = int(cd.sum())
    pc = 0.05 + 0.9 * torch.rand(S, generator=g)
    pc[::5] = 0.0
    pc[3::7] = NAN
    ec = 0.05 + 0.9 * torch.rand(S, generator=g)
    ec[1::6] = NAN
    return Prosody(pitch_contour=pc, energy_contour=ec, contour_durations=cd, pitch_scale=0.8, pitch_shift=0.1, energy_scale=0.9)


def test_a_contour_that_moves_inside_a_phoneme_gives_the_oracles_buckets(world):
    d, e, ids, st = world
    P = e.arena.P
    base, binfo = e.generate_batch(ids, st, want_info=True, **KW)
    for b, n in enumerate(SIZES):
        pr = _varying(n, binfo["durations"][b], 30 + b)
        flat = Prosody(pitch_scale=0.8, pitch_shift=0.1, energy_scale=0.9)
        (mel,), info = e.generate_batch([ids[b]], [st[b]], want_info=True, prosody=[pr], **KW)      # alone: its buffers stay in syn.*
        T = info["T"][0]
        assert torch.equal(info["durations"][0], binfo["durations"][b]), "a contour leaves the durations alone"
        pitch, energy = e._buf("syn.out.pitch", 1, T).cpu(), e._buf("syn.out.energy", 1, T).cpu()
        idx, lens = e._buf("syn.lr.idx", 1, T, dtype=torch.int64).cpu(), e._buf("syn.lr.lens", 1, dtype=torch.int64).cpu()
        pidx, eidx = e._buf("syn.va.pidx", 1, T, dtype=torch.int32).cpu().long(), e._buf("syn.va.eidx", 1, T, dtype=torch.int32).cpu().long()
        t, c = pack([pr], [n], n), pack_contours([pr], [n], n)
        want_p, want_e = PT.contour(pitch, energy, idx, lens, t.pitch_ss[0], t.pitch_ss[1], t.energy_ss[0], t.energy_ss[1], t.pitch, t.energy,
                                    info["durations"][0].cpu()[None], c.src_dur, c.pitch, c.energy)
        live = int(lens[0])
        assert live == int(info["durations"][0].sum()) and live > 0
        assert torch.equal(pidx[0, :live], torch.bucketize(want_p, P[f"{VA}.pitch_bins"].cpu())[0, :live]), f"row {b}: pitch buckets"
        assert torch.equal(eidx[0, :live], torch.bucketize(want_e, P[f"{VA}.energy_bins"].cpu())[0, :live]), f"row {b}: energy buckets"
        (fmel,), _ = e.generate_batch([ids[b]], [st[b]], want_info=True, prosody=[flat], **KW)
        fpidx = e._buf("syn.va.pidx", 1, T, dtype=torch.int32).cpu().long()
        assert not torch.equal(fpidx[0, :live], pidx[0, :live]), f"row {b}: the contour moves the buckets"
        assert fmel.shape != mel.shape or not torch.equal(fmel, mel), f"row {b}: and the mel"
        k = int(torch.argmax(info["durations"][0])) if b else 0
        if int(info["durations"][0][k]) > 1:
            lo = int(info["durations"][0][:k].sum())
            assert len(set(want_p[0, lo:lo + int(info["durations"][0][k])].tolist())) > 1, "the values differ inside one phoneme"


def test_rows_with_contours_equal_the_rows_alone_in_all_three_entry_points(world):
    d, e, ids, st = world
    base = e.generate_batch(ids, st, want_info=True, **KW)[1]
    dur = [x.cpu() for x in base["durations"]]
    g = torch.Generator().manual_seed(9)
    forced = [torch.randint(0, 4, (n,), generator=g) + 2 * (torch.arange(n) == 0) for n in SIZES]
    prosody = [_varying(SIZES[0], dur[0], 50),                                          # on the model's durations
               Prosody.from_tracks(forced[1], torch.rand(int(forced[1].sum()) + 3, generator=g), torch.rand(int(forced[1].sum()) - 2, generator=g)),
               Prosody(speed=1.6, energy=[0.61 if j % 2 else NAN for j in range(SIZES[2])])]   # a row without a contour
    alone = [e.generate_batch([ids[b]], [st[b]], want_info=True, prosody=[prosody[b]], **KW) for b in range(3)]
    mels, info = e.generate_batch(ids, st, want_info=True, prosody=prosody, **KW)
    smels, sinfo = e.generate_stream(ids, st, slots=2, want_info=True, prosody=prosody, **KW)       # the third row is a refill
    salone = [e.generate_stream([ids[b]], [st[b]], slots=2, want_info=True, prosody=[prosody[b]], **KW) for b in range(3)]
    rev, rinfo = e.generate_batch(ids[::-1], st[::-1], want_info=True, prosody=prosody[::-1], **KW)
    for b in range(3):
        for (m, i), (am, ai) in (((mels, info), alone[b]), ((smels, sinfo), salone[b])):
            assert torch.equal(m[b], am[0]), f"row {b}"
            assert torch.equal(i["durations"][b], ai["durations"][0]) and i["T"][b] == ai["T"][0] and i["bounds"][b] == ai["bounds"][0]
        assert torch.equal(rev[2 - b], mels[b]), f"row {b} in another order"
        assert torch.equal(info["durations"][b], sinfo["durations"][b]) and info["bounds"][b] == sinfo["bounds"][b]
        torch.testing.assert_close(smels[b], mels[b], atol=1e-4, rtol=0)
    assert info["durations"][1].tolist() == forced[1].tolist()
    for b in (0, 1):                                                # generate at B = 1: the same row
        one = e.generate(ids[b][None], st[b][None], prosody=prosody[b], **KW)[0]
        assert one.shape == mels[b].shape
        torch.testing.assert_close(one, mels[b], atol=2e-4, rtol=0)       # (each is within 1e-4 of the reference: test_prosody_gpu.py)
    plain = e.generate_batch(ids, st, prosody=[Prosody(), Prosody(durations=forced[1]), prosody[2]], **KW)
    assert not torch.equal(plain[0], mels[0]) and not torch.equal(plain[1], mels[1]) and torch.equal(plain[2], mels[2])


# ---- 3. kokoro-eval --oracle-prosody ----------------------------------------------------------------------------------------------

def test_kokoro_eval_oracle_prosody(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.cli import evaluate as cli
    from kokoro.data.cached import FEATURE_CACHE_VERSION
    from kokoro.training.checkpoint import save_checkpoint
    from kokoro.training.config import TrainingConfig
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d = ModelDims(vocab=59, mel=80, hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32, var_kernel=3,
                  var_bins=16, max_len=300)
    e = KokoroEngine(d, StepHyper(), math_mode="f32", total_steps=100, seed=5)
    cfg = TrainingConfig(n_mels=80, hidden_dim=128, n_encoder_layers=1, n_decoder_layers=1, n_heads=2, encoder_ff_dim=96,
                         decoder_ff_dim=96, max_decoder_seq_len=300, variance_filter_size=32, n_variance_bins=16)
    ck = save_checkpoint(e, cfg, 0, 1.0, str(tmp_path / "ck"))
    g = torch.Generator().manual_seed(4)

    def write(cache):
        cache.mkdir()
        for i, (P, T) in enumerate([(5, 20), (9, 31), (7, 26)]):
            dur = torch.ones(P, dtype=torch.int64)
            dur[-1] = T - (P - 1)
            torch.save({"mel_spec": torch.randn(80, T, generator=g) - 5.0, "phoneme_indices": torch.randint(1, 59, (P,), generator=g),
                        "stress_indices": torch.zeros(P, dtype=torch.int64), "phoneme_durations": dur, "stop_token_targets": torch.zeros(T),
                        "pitch": torch.rand(T, generator=g) * (torch.rand(T, generator=g) > 0.3), "energy": torch.rand(T, generator=g),
                        "mel_length": T, "phoneme_length": P, "text": "", "audio_file": f"u{i}.wav", "_cache_version": FEATURE_CACHE_VERSION},
                       cache / f"u{i}.pt")

    write(tmp_path / "cache")
    base = ["--checkpoint", str(ck), "--features", str(tmp_path / "cache"), "--split", "all", "--math", "f32", "--weights", "model",
            "--max-len", "40", "--min-len-floor", "8", "--slots", "2"]
    plain, forced = tmp_path / "plain.json", tmp_path / "forced.json"
    assert cli.main(base + ["--output", str(plain)]) == 0
    out_plain = capsys.readouterr().out
    assert cli.main(base + ["--output", str(forced), "--oracle-prosody"]) == 0
    out_forced = capsys.readouterr().out
    rp, rf = json.loads(plain.read_text()), json.loads(forced.read_text())
    assert "oracle_prosody" not in rp and "oracle_durations" not in rp, "without the flag: the report it always wrote"
    assert set(rf) == set(rp) | {"oracle_durations", "oracle_prosody"} and rf["oracle_prosody"] is True and rf["oracle_durations"] is True
    assert set(rf["summary"]) == set(rp["summary"]) and [set(r) for r in rf["records"]] == [set(r) for r in rp["records"]]
    assert [r["dur_abs_err"] for r in rf["records"]] == [0.0, 0.0, 0.0] and rf["summary"]["dur_abs_err"]["mean"] == 0.0
    assert [ln.split()[0] for ln in out_forced.splitlines()[1:5]] == [ln.split()[0] for ln in out_plain.splitlines()[1:5]]
