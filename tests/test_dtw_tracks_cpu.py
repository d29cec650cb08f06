"""CPU suite: the fp64 oracle of kk_dtw_track_stats (kokoro_ruslan_amd.dtw_torch.track_stats) against a hand-written loop and on cases
whose answer is known, evaluate()'s audio metrics on a stub engine, vocoder and extractor with an aligner made of the oracle, and the
new flags of the kokoro-eval command line."""
import math

import numpy as np
import pytest
import torch

from kokoro.cli import evaluate as cli
from kokoro.inference import evaluate as E
from kokoro_ruslan_amd import dtw_torch as R

F_LO, F_SPAN = 50.0, 750.0 + 1e-8


def _loop_stats(path, pa, pb, ea, eb, f_lo, f_span, ratio):
    """The definitions, step by step, in Python floats."""
    out = dict(n_vv=0, n_vu=0, n_uv=0, n_uu=0, n_gpe=0, cents_sum=0.0, cents_sq_sum=0.0, energy_l1_sum=0.0)
    for i, j in path:
        p, q = float(pa[i]), float(pb[j])
        out["energy_l1_sum"] += abs(float(ea[i]) - float(eb[j]))
        if p > 0 and q > 0:
            fa, fb = f_lo + f_span * p, f_lo + f_span * q
            c = 1200.0 * math.log2(fa / fb)
            out["n_vv"] += 1
            out["cents_sum"] += c
            out["cents_sq_sum"] += c * c
            if abs(fa - fb) > ratio * fb:
                out["n_gpe"] += 1
        elif p > 0:
            out["n_vu"] += 1
        elif q > 0:
            out["n_uv"] += 1
        else:
            out["n_uu"] += 1
    return out


def _gpe_edge(q, ratio=0.2):
    """(the largest p whose frequency is no gross pitch error against q's, the next double: the first that is one)."""
    fb = F_LO + F_SPAN * q
    p = (fb * (1 + ratio) - F_LO) / F_SPAN
    is_gpe = lambda x: abs((F_LO + F_SPAN * x) - fb) > ratio * fb
    while is_gpe(p):
        p = np.nextafter(p, 0.0)
    while not is_gpe(np.nextafter(p, 1.0)):
        p = np.nextafter(p, 1.0)
    return float(p), float(np.nextafter(p, 1.0))


def test_track_stats_equal_the_hand_written_loop():
    near, far = _gpe_edge(0.2)
    pa = np.array([0.1, near, far, 0.0, 0.31])                                  # 5 frames
    pb = np.array([0.12, 0.2, 0.2, 0.2, 0.0, 0.0, 0.29])                        # 7 frames
    ea, eb = np.array([0.0, 0.25, 1.0, 0.5, 0.125]), np.array([0.5, 0.25, 0.0, 0.75, 0.375, 1.0, 0.0625])
    path = [(0, 0), (1, 1), (1, 2), (2, 3), (3, 3), (3, 4), (3, 5), (4, 5), (4, 6)]
    got = R.track_stats(path, pa, pb, ea, eb, F_LO, F_SPAN, 0.2)
    want = _loop_stats(path, pa, pb, ea, eb, F_LO, F_SPAN, 0.2)
    # by hand: (0,0) vv; (1,1), (1,2) vv on the near side; (2,3) vv on the far side: the one gross error; (3,3) uv; (3,4), (3,5) uu;
    # (4,5) vu; (4,6) vv
    assert (want["n_vv"], want["n_vu"], want["n_uv"], want["n_uu"], want["n_gpe"]) == (5, 1, 1, 2, 1)
    for k in R.TRACK_COUNTS:
        assert got[k] == want[k] and isinstance(got[k], int), k
    for k in R.TRACK_SUMS:
        assert got[k] == pytest.approx(want[k], rel=1e-13), k
    assert got["energy_l1_sum"] == 0.5 + 0 + 0.25 + 0.25 + 0.25 + 0.125 + 0.5 + 0.875 + 0.0625
    m = R.track_metrics(got, len(path))
    assert m["gpe"] == 1 / 5 and m["vuv_err"] == 2 / 9 and m["energy_l1_dtw"] == got["energy_l1_sum"] / 9
    assert m["f0_bias_cents"] == got["cents_sum"] / 5 and m["f0_rmse_cents"] == math.sqrt(got["cents_sq_sum"] / 5)
    assert {k: m[k] for k in R.TRACK_COUNTS} == {k: got[k] for k in R.TRACK_COUNTS}
    # a wider ratio takes the far side in, a ratio of 0 calls every differing pair gross
    assert R.track_stats(path, pa, pb, ea, eb, F_LO, F_SPAN, 0.21)["n_gpe"] == 0
    assert R.track_stats(path, pa, pb, ea, eb, F_LO, F_SPAN, 0.0)["n_gpe"] == 5


def test_identical_tracks_on_the_diagonal_cost_nothing():
    g = np.random.default_rng(0)
    p = np.where(g.random(40) < 0.4, 0.0, g.random(40)).astype(np.float32)
    e = g.random(40).astype(np.float32)
    s = R.track_stats([(i, i) for i in range(40)], p, p, e, e)
    assert s["cents_sum"] == 0.0 and s["cents_sq_sum"] == 0.0 and s["energy_l1_sum"] == 0.0
    assert s["n_vu"] == s["n_uv"] == s["n_gpe"] == 0 and s["n_vv"] == int((p > 0).sum()) and s["n_vv"] + s["n_uu"] == 40
    m = R.track_metrics(s, 40)
    assert m["f0_rmse_cents"] == 0.0 and m["f0_bias_cents"] == 0.0 and m["gpe"] == 0.0 and m["vuv_err"] == 0.0


def test_a_semitone_is_a_hundred_cents():
    """fp32 rounding of p moves f by at most 750 2^-24 = 4.5e-5 Hz: under 1e-3 cents at 80 Hz."""
    g = np.random.default_rng(1)
    fa = 80.0 * 2.0 ** (g.random(200) * math.log2(400.0 / 80.0))                 # 80-400 Hz
    fb = fa * 2.0 ** (-1.0 / 12.0)
    assert fb.min() > 75.0
    pa, pb = ((fa - F_LO) / F_SPAN).astype(np.float32), ((fb - F_LO) / F_SPAN).astype(np.float32)
    s = R.track_stats([(i, i) for i in range(200)], pa, pb, np.zeros(200), np.ones(200))
    m = R.track_metrics(s, 200)
    assert s["n_vv"] == 200 and s["n_gpe"] == 0
    assert abs(m["f0_bias_cents"] - 100.0) <= 0.01 and abs(m["f0_rmse_cents"] - 100.0) <= 0.01 and m["energy_l1_dtw"] == 1.0


def test_no_step_voiced_on_both_sides_gives_none():
    s = R.track_stats([(0, 0), (1, 1)], [0.5, 0.0], [0.0, 0.5], [0.0, 0.0], [0.0, 0.0])
    m = R.track_metrics(s, 2)
    assert m["f0_rmse_cents"] is None and m["f0_bias_cents"] is None and m["gpe"] is None and m["vuv_err"] == 1.0 and m["n_vv"] == 0


# ---- evaluate() on stubs --------------------------------------------------------------------------------------------------------

class StubEngine:
    """Utterance u -> a mel of sum(u) frames whose value rises with the frame; bound = (1, sum(u), 100)."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def _run(self, utterances):
        mels = [torch.arange(int(u.sum()), dtype=torch.float32)[:, None].repeat(1, 4) * 0.1 - float(u.numel()) for u in utterances]
        info = {"durations": [u.clone().float() for u in utterances], "T": [int(u.sum()) for u in utterances],
                "bounds": [(1, int(u.sum()), 100) for u in utterances]}
        return mels, info

    def generate_batch(self, utterances, stress=None, *, want_info=False, **kw):
        self.calls.append(("batch", len(utterances), kw))
        return self._run(utterances)

    def generate_stream(self, utterances, stress=None, *, slots=32, want_info=False, **kw):
        self.calls.append(("stream", len(utterances), slots, kw))
        return self._run(utterances)


class OracleAligner:
    """MelAligner's records from the fp64 oracle alone; keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def align(self, syn, ref, **kw):
        self.calls.append(dict(kw))
        tracks = kw.get("tracks")
        out = []
        for i, (s, r) in enumerate(zip(syn, ref)):
            ca, cb = R.mcep(s, 3), R.mcep(r, 3)
            total, path, _ = R.dtw(ca, cb)
            mcd, l1 = R.path_stats(ca, cb, s, r, path)
            rec = {"total": total, "steps": len(path), "mcd_dtw": mcd / len(path), "mel_l1_dtw": l1 / len(path), "len_ratio": len(s) / len(r)}
            if tracks is not None:
                (pa, pb), (ea, eb) = tracks["pitch"], tracks["energy"]
                assert len(pa[i]) >= len(s) and len(pb[i]) == len(r)
                rec.update(R.track_metrics(R.track_stats(path, pa[i][:len(s)], pb[i], ea[i][:len(s)], eb[i]), len(path)))
            out.append(rec)
        return out


class StubVocoder:
    """A mel of T frames -> 256 T samples, all equal to minus the mel's first value = the utterance's phoneme count (so the extractor
    can tell the utterances apart)."""

    def __init__(self):
        self.calls = []

    def vocode(self, mels, **kw):
        self.calls.append((len(mels), kw, [float(m.max()) for m in mels]))
        return [torch.full((256 * m.shape[0],), -float(m[0, 0])) for m in mels]


class StubDenoiser:
    def __init__(self):
        self.calls = []

    def denoise(self, waves, strength=0.005):
        self.calls.append((len(waves), strength))
        return [w + 100.0 for w in waves]


class StubExtractor:
    """T + 1 feature frames for 256 T samples: the canned tracks of the utterance the waveform's value names."""

    def __init__(self, canned):
        self.canned, self.calls = canned, []

    def extract(self, waves, max_seq_length=1800, **kw):
        self.calls.append((len(waves), max_seq_length))
        out = []
        for w in waves:
            p, e = self.canned[int(round(float(w[0]))) % 100]
            assert p.numel() == w.numel() // 256 + 1
            out.append({"pitch": p, "energy": e, "mel_length": p.numel()})
        return out


UTTS = [torch.tensor([3, 4, 5]), torch.tensor([7]), torch.tensor([1, 2, 2, 1]), torch.tensor([6, 4])]       # 12, 7, 6, 10 frames
REF_T = [10, 7, 8, 10]


def _world():
    g = torch.Generator().manual_seed(0)
    refs = [torch.arange(t, dtype=torch.float32)[:, None].repeat(1, 4) * 0.1 - float(u.numel()) for t, u in zip(REF_T, UTTS)]
    track = lambda n: torch.where(torch.rand(n, generator=g) < 0.3, torch.zeros(n), 0.1 + 0.5 * torch.rand(n, generator=g))
    canned = {int(u.numel()): (track(int(u.sum()) + 1), torch.rand(int(u.sum()) + 1, generator=g)) for u in UTTS}
    ref_pitch, ref_energy = [track(t) for t in REF_T], [torch.rand(t, generator=g) for t in REF_T]
    ref_pitch[1], ref_energy[1] = torch.zeros(7), torch.zeros(7)                        # utterance 1: a cache without variance
    ref_pitch[2] = torch.zeros(8)                                                       # utterance 2: never voiced, but it has energy
    return refs, canned, ref_pitch, ref_energy


TRACK_KEYS = {"f0_rmse_cents", "f0_bias_cents", "gpe", "vuv_err", "energy_l1_dtw", "n_vv", "n_vu", "n_uv", "n_uu", "n_gpe"}
OLD_KEYS = {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw", "mel_l1_dtw", "hit_bound"}


@pytest.mark.parametrize("stream", [True, False])
def test_evaluate_with_a_vocoder_adds_the_track_metrics(stream):
    refs, canned, ref_pitch, ref_energy = _world()
    e, al, voc, ex = StubEngine(), OracleAligner(), StubVocoder(), StubExtractor(canned)
    recs, summ, audio = E.evaluate(e, UTTS, None, refs, stream=stream, slots=3, batch_size=3, aligner=al, vocoder=voc,
                                   vocoder_kwargs={"n_iter": 4}, extractor=ex, ref_pitch=ref_pitch, ref_energy=ref_energy, want_audio=True)
    assert len(voc.calls) == 1 and voc.calls[0][0] == 4 and voc.calls[0][1] == {"n_iter": 4}, "all mels in one vocode() call"
    assert ex.calls == [(4, 4097)] and len(al.calls) == 1 and set(al.calls[0]) == {"tracks"}
    assert [a.numel() for a in audio] == [256 * 12, 256 * 7, 256 * 6, 256 * 10]
    assert [set(r) for r in recs] == [OLD_KEYS | TRACK_KEYS | {"no_variance"}, OLD_KEYS | {"no_variance"},
                                      OLD_KEYS | TRACK_KEYS | {"no_variance"}, OLD_KEYS | TRACK_KEYS | {"no_variance"}]
    assert [r["no_variance"] for r in recs] == [False, True, False, False]
    for i in (0, 2, 3):                                            # every field is the oracle's on the canned tracks cut to the mel
        s, r = e._run([UTTS[i]])[0][0], refs[i]
        _, path, _ = R.dtw(R.mcep(s, 3), R.mcep(r, 3))
        p, en = canned[int(UTTS[i].numel())]
        want = R.track_metrics(R.track_stats(path, p[:len(s)], ref_pitch[i], en[:len(s)], ref_energy[i]), len(path))
        assert {k: recs[i][k] for k in TRACK_KEYS} == want
    assert recs[2]["n_vv"] == 0 and recs[2]["f0_rmse_cents"] is None and recs[2]["gpe"] is None and recs[2]["energy_l1_dtw"] > 0
    assert recs[0]["n_vv"] > 0 and recs[3]["n_vv"] > 0
    # the summary: None and absent values are skipped, the cache entries without variance counted
    assert summ["no_variance"] == 1 and summ["utterances"] == 4
    rm = [recs[i]["f0_rmse_cents"] for i in (0, 3)]
    assert summ["f0_rmse_cents"]["mean"] == pytest.approx(sum(rm) / 2) and summ["gpe"]["mean"] == pytest.approx((recs[0]["gpe"] + recs[3]["gpe"]) / 2)
    assert summ["vuv_err"]["mean"] == pytest.approx(sum(recs[i]["vuv_err"] for i in (0, 2, 3)) / 3)
    assert summ["energy_l1_dtw"]["median"] == pytest.approx(float(np.median([recs[i]["energy_l1_dtw"] for i in (0, 2, 3)])))
    assert set(E.METRICS) >= {"f0_rmse_cents", "f0_bias_cents", "gpe", "vuv_err", "energy_l1_dtw"} and E.METRICS[:4] == ("mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err")


def test_the_denoiser_sits_between_vocoder_and_extractor():
    refs, canned, ref_pitch, ref_energy = _world()
    den = StubDenoiser()
    ex = StubExtractor(canned)                                                    # (w + 100: the same utterance number modulo 100)
    recs, summ = E.evaluate(StubEngine(), UTTS, None, refs, aligner=OracleAligner(), vocoder=StubVocoder(), denoiser=den,
                            denoise_strength=0.25, extractor=ex, ref_pitch=ref_pitch, ref_energy=ref_energy)
    assert den.calls == [(4, 0.25)] and ex.calls == [(4, 4097)] and "f0_rmse_cents" in recs[0]


def test_summarize_skips_none_and_leaves_out_what_no_record_has():
    recs = [{"hit_bound": False, "gpe": None, "vuv_err": 0.5, "no_variance": False}, {"hit_bound": True, "gpe": 0.25, "vuv_err": 0.0, "no_variance": False},
            {"hit_bound": False, "no_variance": True}]
    s = E.summarize(recs)
    assert s["gpe"] == {"mean": 0.25, "median": 0.25, "p95": 0.25} and s["vuv_err"]["mean"] == 0.25 and s["no_variance"] == 1
    assert "f0_rmse_cents" not in s and "mcd_dtw" not in s
    s = E.summarize([{"hit_bound": False, "gpe": None, "no_variance": False}])
    assert "gpe" not in s and s["no_variance"] == 0
    assert "no_variance" not in E.summarize([{"hit_bound": False, "mcd_dtw": 1.0}])


def test_without_a_vocoder_nothing_changes():
    refs, *_ = _world()
    e1, e2, a1, a2 = StubEngine(), StubEngine(), OracleAligner(), OracleAligner()
    durs = [u + 1 for u in UTTS]
    old = E.evaluate(e1, UTTS, None, refs, slots=3, durations=durs, names=list("abcd"), aligner=a1, max_len=50)
    new = E.evaluate(e2, UTTS, None, refs, slots=3, durations=durs, names=list("abcd"), aligner=a2, max_len=50, vocoder=None,
                     vocoder_kwargs=None, denoiser=None, denoise_strength=0.005, extractor=None, ref_pitch=None, ref_energy=None,
                     want_audio=False)
    assert old == new and len(new) == 2 and e1.calls == e2.calls == [("stream", 4, 3, {"max_len": 50})]
    assert a1.calls == a2.calls == [{}], "align() is called as it always was: no tracks keyword"
    assert all(set(r) == OLD_KEYS | {"dur_abs_err"} for r in new[0]) and "no_variance" not in new[1]
    assert set(new[1]) == {"utterances", "hit_bound_share", "mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err"}


def test_argument_errors_of_the_audio_metrics():
    refs, canned, ref_pitch, ref_energy = _world()
    e = StubEngine()
    base = dict(aligner=OracleAligner(), extractor=StubExtractor(canned))
    ok = dict(vocoder=StubVocoder(), ref_pitch=ref_pitch, ref_energy=ref_energy)
    with pytest.raises(ValueError, match="ref_pitch and ref_energy"):
        E.evaluate(e, UTTS, None, refs, vocoder=StubVocoder(), **base)
    with pytest.raises(ValueError, match="ref_pitch and ref_energy"):
        E.evaluate(e, UTTS, None, refs, vocoder=StubVocoder(), ref_pitch=ref_pitch, **base)
    with pytest.raises(ValueError, match="ref_pitch and ref_energy"):
        E.evaluate(e, UTTS, None, refs, vocoder=StubVocoder(), ref_energy=ref_energy, **base)
    with pytest.raises(ValueError, match="ref_pitch: 3 entries for 4"):
        E.evaluate(e, UTTS, None, refs, **dict(ok, ref_pitch=ref_pitch[:3]), **base)
    with pytest.raises(ValueError, match="ref_energy: 5 entries for 4"):
        E.evaluate(e, UTTS, None, refs, **dict(ok, ref_energy=ref_energy + ref_energy[:1]), **base)
    with pytest.raises(ValueError, match="vocoder_kwargs must be a dict"):
        E.evaluate(e, UTTS, None, refs, vocoder_kwargs=[4], **ok, **base)
    for bad in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="denoise_strength"):
            E.evaluate(e, UTTS, None, refs, denoiser=StubDenoiser(), denoise_strength=bad, **ok, **base)
    for kw in (dict(ref_pitch=ref_pitch), dict(ref_energy=ref_energy), dict(denoiser=StubDenoiser()), dict(vocoder_kwargs={}),
               dict(extractor=StubExtractor(canned)), dict(want_audio=True)):
        with pytest.raises(ValueError, match="needs a vocoder"):
            E.evaluate(e, UTTS, None, refs, aligner=OracleAligner(), **kw)
    assert e.calls == [], "every argument error comes before the synthesis"
    assert E.evaluate(e, [], None, [], want_audio=True, **dict(ok, ref_pitch=[], ref_energy=[]), **base) == ([], {"utterances": 0, "hit_bound_share": 0.0}, [])


def test_aligner_track_guards_need_no_device():
    from kokoro_ruslan_amd.dtw import MelAligner
    a = MelAligner(device="cpu")
    m, t = (lambda n: torch.zeros(n, 8)), (lambda n: torch.zeros(n))
    tr = lambda pa, pb, ea, eb: {"pitch": ([pa], [pb]), "energy": ([ea], [eb])}
    with pytest.raises(ValueError, match="pair 0: the synthesized pitch track has 4 entries for 5 frames"):
        a.align([m(5)], [m(3)], tracks=tr(t(4), t(3), t(5), t(3)))
    with pytest.raises(ValueError, match="pair 0: the synthesized energy track has 2 entries for 5 frames"):
        a.align([m(5)], [m(3)], tracks=tr(t(6), t(3), t(2), t(3)))
    with pytest.raises(ValueError, match="pair 0: the reference pitch track has 4 entries for 3 frames"):
        a.align([m(5)], [m(3)], tracks=tr(t(5), t(4), t(5), t(3)))
    with pytest.raises(ValueError, match="pair 0: the reference energy track has 2 entries for 3 frames"):
        a.align([m(5)], [m(3)], tracks=tr(t(5), t(3), t(5), t(2)))
    with pytest.raises(ValueError, match="1-D float tensor"):
        a.align([m(5)], [m(3)], tracks=tr(t(5).long(), t(3), t(5), t(3)))
    with pytest.raises(ValueError, match="1-D float tensor"):
        a.align([m(5)], [m(3)], tracks=tr(t(5), t(3)[:, None], t(5), t(3)))
    with pytest.raises(ValueError, match="1-D float tensor"):
        a.align([m(5)], [m(3)], tracks=tr(t(5), t(3), [0.0] * 5, t(3)))
    with pytest.raises(ValueError, match="tracks must be"):
        a.align([m(5)], [m(3)], tracks={"pitch": ([t(5)], [t(3)])})
    with pytest.raises(ValueError, match="2 synthesized tracks for 1 pairs"):
        a.align([m(5)], [m(3)], tracks={"pitch": ([t(5), t(5)], [t(3)]), "energy": ([t(5)], [t(3)])})
    with pytest.raises(ValueError, match="gpe_ratio"):
        MelAligner(device="cpu", gpe_ratio=-0.1)
    assert a.align([], [], tracks={"pitch": ([], []), "energy": ([], [])}) == []


# ---- the CLI --------------------------------------------------------------------------------------------------------------------

BASE = ["--checkpoint", "c", "--features", "d"]


@pytest.mark.parametrize("extra,message", [
    (["--griffin-lim", "--vocoder", "v"], "--griffin-lim and --vocoder are alternatives"),
    (["--griffin-lim-iters", "8"], "--griffin-lim-iters / --griffin-lim-seed need --griffin-lim"),
    (["--griffin-lim-seed", "1"], "--griffin-lim-iters / --griffin-lim-seed need --griffin-lim"),
    (["--vocoder", "v", "--griffin-lim-iters", "8"], "--griffin-lim-iters / --griffin-lim-seed need --griffin-lim"),
    (["--griffin-lim", "--griffin-lim-iters", "-1"], "--griffin-lim-iters must be >= 0"),
    (["--denoise"], "--denoise needs --vocoder"),
    (["--griffin-lim", "--denoise"], "--denoise needs --vocoder"),
    (["--vocoder", "v", "--denoise", "-1"], "--denoise must be >= 0"),
    (["--gpe-ratio", "0.3"], "--gpe-ratio needs --vocoder or --griffin-lim"),
    (["--griffin-lim", "--gpe-ratio", "-0.1"], "--gpe-ratio must be >= 0"),
    (["--vocoder", "v", "--gpe-ratio", "nan"], "--gpe-ratio must be >= 0"),
    (["--vocoder", "v", "--vocoder-math", "fp8"], "argument --vocoder-math: invalid choice: 'fp8'")])
def test_conflicting_flags_go_through_parser_error(extra, message, capsys):
    """Each conflict ends in parser.error with the message of its own guard (exit code 2, the usage line first)."""
    p = cli.build_parser()
    with pytest.raises(SystemExit) as ex:
        cli.check_args(p, p.parse_args(BASE + extra))
    err = capsys.readouterr().err
    assert ex.value.code == 2 and err.startswith("usage:") and f"error: {message}" in err


def test_the_griffin_lim_model_check_is_kokoro_synths(capsys):
    from kokoro.cli import synth
    p = cli.build_parser()
    synth.check_vocoder_model(p, p.parse_args(BASE + ["--griffin-lim"]), 80)
    synth.check_vocoder_model(p, p.parse_args(BASE + ["--vocoder", "v"]), 20)
    with pytest.raises(SystemExit) as ex:
        synth.check_vocoder_model(p, p.parse_args(BASE + ["--griffin-lim"]), 20)
    assert ex.value.code == 2 and "error: --griffin-lim needs an 80-mel model; this checkpoint makes 20 mel channels" in capsys.readouterr().err


def test_parser_defaults_and_the_new_flags():
    p = cli.build_parser()
    a = p.parse_args(BASE)
    cli.check_args(p, a)
    assert (a.split, a.validation_split, a.weights, a.math, a.no_stream, a.slots, a.batch_size, a.mcep, a.output) == \
        (None, 0.1, "auto", "bf16", False, None, None, 13, None)
    assert (a.stop_threshold, a.max_len, a.min_len_ratio, a.min_len_floor, a.oracle_durations) == (None, None, None, None, False)
    assert (a.vocoder, a.vocoder_config, a.vocoder_math, a.denoise, a.griffin_lim, a.griffin_lim_iters, a.griffin_lim_seed, a.gpe_ratio) == \
        (None, None, "bf16", None, False, 60, None, 0.2)
    a = p.parse_args(BASE + ["--vocoder", "v", "--vocoder-math", "f32", "--denoise", "--gpe-ratio", "0.1"])
    cli.check_args(p, a)
    assert (a.vocoder, a.vocoder_math, a.denoise, a.gpe_ratio) == ("v", "f32", 0.005, 0.1)
    a = p.parse_args(BASE + ["--griffin-lim", "--griffin-lim-iters", "8", "--griffin-lim-seed", "3"])
    cli.check_args(p, a)
    assert (a.griffin_lim, a.griffin_lim_iters, a.griffin_lim_seed) == (True, 8, 3)
    # the same spelling as kokoro-synth: one definition
    from kokoro.cli import synth
    s = synth.build_parser().parse_args(["--checkpoint", "c", "--features", "d", "--output", "o"])
    for k in ("vocoder", "vocoder_config", "vocoder_math", "denoise", "griffin_lim", "griffin_lim_iters", "griffin_lim_seed"):
        assert getattr(s, k) == getattr(p.parse_args(BASE), k), k
