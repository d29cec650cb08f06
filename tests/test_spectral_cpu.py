"""CPU suite: the fp64 oracle of the spectral distance (kokoro_ruslan_amd.spectral_torch) against an independent formulation with
torch.stft and on cases whose answer is known, the argument checks of SpectralDistance and evaluate() that need no device, and the new
flags of the kokoro-eval command line."""
import math

import pytest
import torch

from kokoro.cli import evaluate as cli
from kokoro.inference import evaluate as E
from kokoro_ruslan_amd import features_torch as FT
from kokoro_ruslan_amd import spectral_torch as R
from kokoro_ruslan_amd.stft import HOP, N_FFT, centred_hann_windows, hann_window

N_A, N_B = 6000, 7000                                    # 24 and 28 frames


@pytest.fixture(scope="module")
def pair():
    a, b = FT.test_signal(N_A, seed=0, f0=120.0), FT.test_signal(N_B, seed=1, f0=150.0)
    Ta, Tb = 1 + N_A // HOP, 1 + N_B // HOP
    path, i, j = [], 0, 0                                # a monotone path with all three step kinds
    while True:
        path.append((i, j))
        if i == Ta - 1 and j == Tb - 1:
            break
        kind = len(path) % 3
        if i == Ta - 1 or (kind == 1 and j < Tb - 1):
            j += 1
        elif j == Tb - 1 or kind == 2:
            i += 1
        else:
            i, j = i + 1, j + 1
    return a, b, torch.tensor(path), Ta, Tb


def _stft_sums(a, b, path, dtype=torch.float64):
    """The fifteen sums from torch.stft with win_length = w (which centres the window itself) and gathers along the path."""
    a, b = FT.normalise(a, dtype), FT.normalise(b, dtype)
    rows = []
    for w in R.WINDOWS:
        win = torch.hann_window(w, periodic=True, dtype=dtype)
        A, B = (torch.stft(x, N_FFT, HOP, w, win, center=True, pad_mode="reflect", onesided=True, return_complex=True).abs().double()
                for x in (a, b))
        A, B = A[:, path[:, 0]], B[:, path[:, 1]]
        d = 10.0 * torch.log10((A * A + 1e-9) / (B * B + 1e-9))
        rows.append(torch.stack([(A * B).sum(), (A * A).sum(), (B * B).sum(), d.sum(), (d * d).sum()]))
    return torch.stack(rows)


def test_window_tables():
    w = centred_hann_windows(torch.float64)
    assert w.shape == (3, N_FFT) and torch.equal(w[2], hann_window(torch.float64))
    for r, n in enumerate((256, 512, 1024)):
        lo, hi = 512 - n // 2, 512 + n // 2
        assert torch.equal(w[r, lo:hi], torch.hann_window(n, periodic=True, dtype=torch.float64))
        assert float(w[r, :lo].abs().sum()) == 0.0 and float(w[r, hi:].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="window width"):
        centred_hann_windows(widths=(255,))


def test_oracle_agrees_with_torch_stft(pair):
    a, b, path, Ta, Tb = pair
    got = R.spectral_stats(a, b, path, Ta, Tb)
    want = _stft_sums(a, b, path)
    assert got["steps"] == len(path) and got["skipped"] == 0 and got["sums"].dtype == torch.float64
    rel = ((got["sums"] - want).abs() / want.abs()).max()
    print(f"largest relative difference of the fifteen sums: {float(rel):.2e}")
    assert float(rel) <= 1e-12


def test_identical_waveforms_on_the_diagonal_are_zero(pair):
    a, _, _, Ta, _ = pair
    diag = torch.arange(Ta)[:, None].repeat(1, 2)
    m = R.measure(a, a.clone(), diag, Ta, Ta)
    assert m["spec_steps"] == Ta and m["spec_skipped"] == 0
    for k in R.FIELDS:
        assert m[k] == 0.0 and isinstance(m[k], float), k


def test_a_power_of_two_gain_changes_nothing(pair):
    """x / (max|x| + 1e-9) takes a gain g out up to the 1e-9 in the divisor: the scaled side comes out (p + 1e-9) / (p + 1e-9 / g) times
    as large (p the peak), which moves level_db by 8.7 (1 / g - 1) 1e-9 / p dB.  At the unit peak of normalised audio and g = 0.25 that is
    2.6e-8 dB, itself above the 1e-9 asked here, so the waveforms carry the 16-bit PCM scale (x 2^15, exact): 8e-13 dB."""
    a, b, path, Ta, Tb = pair
    a, b = a * 32768.0, b * 32768.0
    one, quarter = R.measure(a, b, path, Ta, Tb), R.measure(0.25 * a, b, path, Ta, Tb)
    for k in R.FIELDS:
        print(f"{k}: {one[k]!r} / {quarter[k]!r}")
        assert abs(one[k] - quarter[k]) <= 1e-9, k
    assert (one["spec_steps"], one["spec_skipped"]) == (quarter["spec_steps"], quarter["spec_skipped"])
    assert one["mr_lsd_dtw"] > 1.0 and one["mr_sc_dtw"] > 0.1, "two different signals: the fields are not trivially zero"


def test_white_noise_raises_the_distances_monotonically(pair):
    a, _, _, Ta, _ = pair
    diag = torch.arange(Ta)[:, None].repeat(1, 2)
    noise = torch.randn(a.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    noise = noise * (a.pow(2).mean().sqrt() / noise.pow(2).mean().sqrt())
    got = [R.measure(a + 10.0 ** (db / 20.0) * noise, a, diag, Ta, Ta) for db in (-40.0, -30.0, -20.0)]
    print([(g["mr_sc_dtw"], g["mr_lsd_dtw"]) for g in got])
    assert 0.0 < got[0]["mr_sc_dtw"] < got[1]["mr_sc_dtw"] < got[2]["mr_sc_dtw"]
    assert 0.0 < got[0]["mr_lsd_dtw"] < got[1]["mr_lsd_dtw"] < got[2]["mr_lsd_dtw"]


def test_bad_steps_are_skipped_and_counted(pair):
    a, b, path, Ta, Tb = pair
    clean = R.spectral_stats(a, b, path, Ta, Tb)
    bad = torch.tensor([[-1, 0], [0, Tb], [Ta, 0], [2 ** 30, 1], [3, -7]])
    got = R.spectral_stats(a, b, torch.cat([path[:5], bad, path[5:]]), Ta, Tb)
    assert got["steps"] == len(path) and got["skipped"] == 5 and torch.equal(got["sums"], clean["sums"])
    # a frame centre beyond the end: the mel says Ta frames, the waveform given is shorter (256 i > n); centre == n is still counted
    short = a[:HOP * 10]                                # frames 0 .. 10 lie within it
    p = torch.tensor([[9, 0], [10, 1], [11, 2], [12, 3]])
    got = R.spectral_stats(short, b, p, Ta, Tb)
    assert (got["steps"], got["skipped"]) == (2, 2)
    m = R.spectral_metrics(got["sums"], got["steps"], got["skipped"])
    assert m["spec_steps"] == 2 and m["spec_skipped"] == 2 and math.isfinite(m["mr_lsd_dtw"])
    none = R.measure(a, b, bad, Ta, Tb)
    assert none["spec_steps"] == 0 and none["spec_skipped"] == 5 and all(none[k] is None for k in R.FIELDS)


def test_a_silent_side_has_no_convergence(pair):
    a, _, _, Ta, _ = pair
    diag = torch.arange(Ta)[:, None].repeat(1, 2)
    m = R.measure(a, torch.zeros(N_A, dtype=torch.float64), diag, Ta, Ta)
    assert m["sc_dtw_1024"] is None and m["mr_sc_dtw"] is None and m["mr_lsd_dtw"] > 0.0 and m["level_db_1024"] > 0.0


def test_oracle_argument_errors(pair):
    a, b, path, Ta, Tb = pair
    with pytest.raises(ValueError, match="samples >= 1024"):
        R.spectral_stats(a[:1023], b, path, Ta, Tb)
    with pytest.raises(ValueError, match="samples >= 1024"):
        R.spectral_stats(a, b[None], path, Ta, Tb)
    with pytest.raises(ValueError, match="at most 8191"):
        R.spectral_stats(a, b, torch.zeros(8192, 2, dtype=torch.int64), Ta, Tb)
    with pytest.raises(ValueError, match="14 sums"):
        R.spectral_metrics([0.0] * 14, 1)


def test_device_class_argument_errors(pair, monkeypatch):
    """SpectralDistance checks everything before its first launch (no device here: the tile constant is given)."""
    from kokoro_ruslan_amd import spectral as S
    monkeypatch.setattr(S, "tile_steps", lambda: 32)
    sd = S.SpectralDistance(device="cpu")
    a, b, path, Ta, Tb = pair
    a, b = a.float(), b.float()
    with pytest.raises(ValueError, match="1 synthesized waveforms for 2 pairs"):
        sd.measure([a], [b, b], [path, path], [Ta, Ta], [Tb, Tb])
    with pytest.raises(ValueError, match="reference waveform has 1023 samples"):
        sd.measure([a], [b[:1023]], [path], [Ta], [Tb])
    with pytest.raises(ValueError, match="1-D float tensor"):
        sd.measure([a.long()], [b], [path], [Ta], [Tb])
    with pytest.raises(ValueError, match="integer tensor"):
        sd.measure([a], [b], [path.float()], [Ta], [Tb])
    with pytest.raises(ValueError, match="integer tensor"):
        sd.measure([a], [b], [path[:, :1]], [Ta], [Tb])
    with pytest.raises(ValueError, match="8192 steps"):
        sd.measure([a], [b], [torch.zeros(8192, 2, dtype=torch.int32)], [Ta], [Tb])
    with pytest.raises(ValueError, match="0 steps"):
        sd.measure([a], [b], [path[:0]], [Ta], [Tb])
    with pytest.raises(ValueError, match="frames must be an integer >= 1"):
        sd.measure([a], [b], [path], [0], [Tb])
    with pytest.raises(ValueError, match="2 reference frame counts"):
        sd.measure([a], [b], [path], [Ta], [Tb, Tb])
    assert sd.measure([], [], [], [], []) == []
    tiles, toff = sd.tiles([31, 32, 33, 65, 0])
    assert toff.tolist() == [0, 1, 2, 4, 7, 7] and tiles.tolist() == [[0, 0], [1, 0], [2, 0], [2, 32], [3, 0], [3, 32], [3, 64]]


# ---- evaluate() ----------------------------------------------------------------------------------------------------------------

class _Engine:
    device = "cpu"

    def __init__(self):
        self.calls = 0

    def generate_stream(self, ids, stress, slots, want_info, **kw):
        self.calls += 1
        mels = [torch.zeros(int(u.sum()), 4) for u in ids]
        return mels, {"durations": [u.float() for u in ids], "T": [m.shape[0] for m in mels], "bounds": [(1, m.shape[0], 100) for m in mels]}


class _Aligner:
    def __init__(self):
        self.calls = []

    def align(self, syn, ref, want_path=False, tracks=None):
        self.calls.append((want_path, tracks is not None))
        out = []
        for s, r in zip(syn, ref):
            rec = {"len_ratio": s.shape[0] / r.shape[0], "mcd_dtw": 1.0, "mel_l1_dtw": 2.0, "steps": 3}
            if tracks is not None:
                rec.update({k: 0.5 for k in E.TRACK_METRICS}, **{k: 1 for k in E.TRACK_COUNTS})
            if want_path:
                rec["path"] = torch.zeros(3, 2, dtype=torch.int32)
            out.append(rec)
        return out


class _Vocoder:
    def vocode(self, mels, **kw):
        return [torch.full((2048,), float(i + 1)) for i, _ in enumerate(mels)]


class _Extractor:
    def extract(self, waves, max_seq_length):
        return [{"pitch": torch.ones(64), "energy": torch.ones(64)} for _ in waves]


class _Spectral:
    def __init__(self):
        self.calls = []

    def measure(self, syn, ref, paths, na, nb):
        self.calls.append(([float(w[0]) for w in syn], [float(w[0]) for w in ref], [tuple(p.shape) for p in paths], list(na), list(nb)))
        return [dict({k: 0.25 * (i + 1) for k in R.FIELDS}, spec_steps=3, spec_skipped=i, extra="dropped") for i in range(len(syn))]


UTTS = [torch.tensor([2, 3]), torch.tensor([4])]


def _audio_kw():
    return dict(vocoder=_Vocoder(), extractor=_Extractor(), ref_pitch=[torch.ones(6), torch.ones(5)], ref_energy=[torch.ones(6), torch.ones(5)])


def test_evaluate_with_ref_waves_adds_the_spectral_fields():
    refs = [torch.zeros(6, 4), torch.zeros(5, 4)]
    al, sp = _Aligner(), _Spectral()
    recs, summ = E.evaluate(_Engine(), UTTS, None, refs, aligner=al, spectral=sp, ref_waves=[torch.full((1500,), 7.0), torch.full((1400,), 8.0)],
                            **_audio_kw())
    assert al.calls == [(True, True)], "one align() call, asked for the paths"
    assert sp.calls == [([1.0, 2.0], [7.0, 8.0], [(3, 2), (3, 2)], [5, 4], [6, 5])], "one measure() call on the vocoded waveforms"
    for i, r in enumerate(recs):
        assert set(E.SPECTRAL_METRICS + E.SPECTRAL_COUNTS) <= set(r) and "extra" not in r
        assert r["mr_sc_dtw"] == 0.25 * (i + 1) and r["spec_skipped"] == i and r["f0_rmse_cents"] == 0.5
    assert summ["mr_lsd_dtw"] == {"mean": 0.375, "median": 0.375, "p95": pytest.approx(0.4875)}
    assert set(E.SPECTRAL_METRICS) <= set(summ) and "spec_steps" not in summ
    assert set(E.SPECTRAL_METRICS) == set(R.FIELDS) and E.SPECTRAL_COUNTS == R.COUNTS


def test_evaluate_without_ref_waves_is_the_parents():
    refs = [torch.zeros(6, 4), torch.zeros(5, 4)]
    al = _Aligner()
    recs, summ = E.evaluate(_Engine(), UTTS, None, refs, aligner=al, **_audio_kw())
    assert al.calls == [(False, True)]
    parent = {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw", "mel_l1_dtw", "hit_bound", "no_variance", "f0_rmse_cents",
              "f0_bias_cents", "gpe", "vuv_err", "energy_l1_dtw", "n_vv", "n_vu", "n_uv", "n_uu", "n_gpe"}
    assert all(set(r) == parent for r in recs)
    assert set(summ) == {"utterances", "hit_bound_share", "mcd_dtw", "mel_l1_dtw", "len_ratio", "f0_rmse_cents", "f0_bias_cents", "gpe",
                         "vuv_err", "energy_l1_dtw", "no_variance"}
    al2 = _Aligner()
    recs2, summ2 = E.evaluate(_Engine(), UTTS, None, refs, aligner=al2)
    assert al2.calls == [(False, False)] and all(set(r) == {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw", "mel_l1_dtw", "hit_bound"}
                                                 for r in recs2)


def test_evaluate_ref_waves_argument_errors():
    refs = [torch.zeros(6, 4), torch.zeros(5, 4)]
    e = _Engine()
    waves = [torch.zeros(1500), torch.zeros(1400)]
    with pytest.raises(ValueError, match="ref_waves needs a vocoder"):
        E.evaluate(e, UTTS, None, refs, aligner=_Aligner(), ref_waves=waves)
    with pytest.raises(ValueError, match="spectral needs a vocoder"):
        E.evaluate(e, UTTS, None, refs, aligner=_Aligner(), spectral=_Spectral())
    with pytest.raises(ValueError, match="spectral needs ref_waves"):
        E.evaluate(e, UTTS, None, refs, aligner=_Aligner(), spectral=_Spectral(), **_audio_kw())
    with pytest.raises(ValueError, match="ref_waves: 1 entries for 2"):
        E.evaluate(e, UTTS, None, refs, aligner=_Aligner(), ref_waves=waves[:1], **_audio_kw())
    with pytest.raises(ValueError, match=r"ref_waves\[1\] must be a 1-D float tensor"):
        E.evaluate(e, UTTS, None, refs, aligner=_Aligner(), ref_waves=[waves[0], waves[1][None]], **_audio_kw())
    assert e.calls == 0, "every argument error comes before the synthesis"


def test_evaluate_vocoder_on_stubs():
    mels = [torch.zeros(6, 4), torch.zeros(5, 4)]
    waves = [torch.full((1500,), 7.0), torch.full((1400,), 8.0)]
    al, sp = _Aligner(), _Spectral()
    recs, summ = E.evaluate_vocoder(_Vocoder(), mels, waves, aligner=al, spectral=sp, names=["a", "b"], device="cpu")
    assert al.calls == [(True, False)] and sp.calls == [([1.0, 2.0], [7.0, 8.0], [(3, 2), (3, 2)], [6, 5], [6, 5])]
    assert all(set(r) == {"name", "frames"} | set(E.SPECTRAL_METRICS + E.SPECTRAL_COUNTS) for r in recs) and recs[1]["name"] == "b"
    assert set(summ) == {"utterances"} | set(E.SPECTRAL_METRICS)
    al = _Aligner()
    recs, summ, audio = E.evaluate_vocoder(_Vocoder(), mels, waves, [torch.ones(6), torch.zeros(5)], [torch.ones(6), torch.zeros(5)], aligner=al,
                                           spectral=_Spectral(), extractor=_Extractor(), device="cpu", want_audio=True)
    assert al.calls == [(True, True)] and len(audio) == 2 and summ["no_variance"] == 1
    assert recs[0]["no_variance"] is False and recs[0]["vuv_err"] == 0.5 and recs[1]["no_variance"] is True and "vuv_err" not in recs[1]
    assert recs[1]["mr_sc_dtw"] == 0.5, "an utterance without tracks still has its spectral fields"
    for kw, msg in ((dict(ref_pitch=[torch.ones(6)] * 2), "both or neither"), (dict(names=["a"]), "names: 1 entries"),
                    (dict(vocoder_kwargs=[1]), "must be a dict"), (dict(denoiser=object(), denoise_strength=-1.0), "denoise_strength")):
        with pytest.raises(ValueError, match=msg):
            E.evaluate_vocoder(_Vocoder(), mels, waves, aligner=_Aligner(), spectral=_Spectral(), device="cpu", **kw)
    with pytest.raises(ValueError, match="needs a vocoder"):
        E.evaluate_vocoder(None, mels, waves)
    with pytest.raises(ValueError, match="needs ref_waves"):
        E.evaluate_vocoder(_Vocoder(), mels, None)
    with pytest.raises(ValueError, match="ref_waves: 1 entries"):
        E.evaluate_vocoder(_Vocoder(), mels, waves[:1], aligner=_Aligner(), spectral=_Spectral(), device="cpu")
    assert E.evaluate_vocoder(_Vocoder(), [], [], device="cpu") == ([], {"utterances": 0, "hit_bound_share": 0.0})


# ---- kokoro-eval ----------------------------------------------------------------------------------------------------------------

BASE = ["--checkpoint", "ck", "--features", "cache"]
FLAGLESS = dict(checkpoint="ck", features="cache", indices=None, split=None, validation_split=0.1, weights="auto", math="bf16", no_stream=False,
                slots=None, batch_size=None, mcep=13, stop_threshold=None, max_len=None, min_len_ratio=None, min_len_floor=None, output=None,
                oracle_durations=False, vocoder=None, vocoder_config=None, vocoder_math="bf16", denoise=None, griffin_lim=False,
                griffin_lim_iters=60, griffin_lim_seed=None, gpe_ratio=0.2)


def _parse(argv):
    p, args = cli.parse(argv)
    cli.check_args(p, args)
    return args


def test_the_flagless_namespace_is_unchanged():
    assert vars(_parse(BASE)) == FLAGLESS
    assert vars(cli.build_parser().parse_args(BASE)) == FLAGLESS


def test_new_flags_parse():
    a = _parse(BASE + ["--griffin-lim", "--wavs", "rec"])
    assert a.wavs == "rec" and not hasattr(a, "copy_synthesis")
    a = _parse(["--features", "cache", "--vocoder", "v", "--denoise", "--wavs", "rec", "--copy-synthesis"])
    assert a.copy_synthesis is True and a.checkpoint is None and a.wavs == "rec" and a.denoise == 0.005
    a = _parse(BASE + ["--griffin-lim", "--wavs", "rec", "--copy-synthesis"])
    assert a.checkpoint == "ck"
    assert "--conditioned-wavs" in cli.build_parser().format_help() and "--conditioned-wavs" in cli.__doc__


@pytest.mark.parametrize("argv, msg", [
    (BASE + ["--wavs", "rec"], "--wavs needs --vocoder or --griffin-lim"),
    (BASE + ["--griffin-lim", "--copy-synthesis"], "--copy-synthesis needs --wavs"),
    (["--features", "cache", "--wavs", "rec", "--copy-synthesis"], "--wavs needs --vocoder or --griffin-lim"),
    (["--features", "cache", "--griffin-lim", "--wavs", "rec"], "the following arguments are required: --checkpoint"),
    (["--features", "cache"], "the following arguments are required: --checkpoint"),
    (["--checkpoint", "ck", "--griffin-lim", "--wavs", "rec", "--copy-synthesis"], "the following arguments are required: --features"),
    (BASE + ["--griffin-lim", "--wavs", "rec", "--copy-synthesis", "--oracle-durations"], "synthesizes nothing"),
    (BASE + ["--griffin-lim", "--vocoder", "v", "--wavs", "rec"], "alternatives"),
])
def test_new_flags_exclusions(argv, msg, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_read_wavs_names_what_is_wrong(tmp_path):
    import numpy as np
    from scipy.io import wavfile
    wavfile.write(str(tmp_path / "u0.wav"), 22050, (np.arange(2048) % 100 * 100).astype(np.int16))
    wavfile.write(str(tmp_path / "u1.wav"), 16000, np.zeros(2048, dtype=np.int16))
    got = cli.read_wavs(str(tmp_path), ["u0"])
    assert len(got) == 1 and got[0].dtype == torch.float32 and got[0].shape == (2048,)
    with pytest.raises(ValueError, match="u2.wav: no such recording"):
        cli.read_wavs(str(tmp_path), ["u0", "u2"])
    with pytest.raises(ValueError, match="u1.wav: sample rate 16000"):
        cli.read_wavs(str(tmp_path), ["u1"])
