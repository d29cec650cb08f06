"""GPU suite: the audio metrics of kokoro.inference.evaluate.evaluate on a tiny random-weight 80-mel engine with Griffin-Lim at 4
iterations from seeded phases (no checkpoint needed): every new record field against the fp64 oracle on tracks the test extracts
itself from the returned waveforms, the stream and batch paths, the exact zero case, the call without a vocoder, the kokoro-eval
command line, and one sanity run on two synthetic harmonic waveforms a whole tone apart."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from kokoro_ruslan_amd import dtw_torch as R
from oracle import kokoro_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dtw_tracks_cases import close, pitch_track  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VA = "duration_adaptor.variance_adaptor"
PHONEMES = (2, 9, 5, 23)
DUR_BIAS = 1.5                         # durations ~ e^1.5 per phoneme: rows of ten to a hundred frames
STOP_AT_MIN = dict(max_len=160, stop_threshold=0.0)       # the stop rule fires on the first frame it may: at the row's minimum length
TRACK_KEYS = ("f0_rmse_cents", "f0_bias_cents", "gpe", "vuv_err", "energy_l1_dtw", "n_vv", "n_vu", "n_uv", "n_uu", "n_gpe")
GL_SEED = 5


def _gl():
    return dict(n_iter=4, generator=torch.Generator().manual_seed(GL_SEED))          # (a generator is used up: a fresh one per call)


def _fixture():                        # (the tiny model of test_evaluate_gpu.py, with the 80 mels Griffin-Lim takes)
    fx = np.load(os.path.join(GOLDEN, "inference_tiny.npz"))
    dims = [int(x) for x in fx["dims"]]
    dims[1] = 80
    d = O.ModelDims(*dims)
    seed = int(fx["seed"])
    P = O.init_params(d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in P.items():
        if p.dim() == 1:
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    P[f"{VA}.duration_predictor.linear.bias"].fill_(DUR_BIAS)
    return d, P


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.inference.audio import vocode
    from kokoro_ruslan_amd.dtw import MelAligner
    from kokoro_ruslan_amd.engine import KokoroEngine
    from kokoro_ruslan_amd.features import FeatureExtractor
    from kokoro_ruslan_amd.griffinlim import GriffinLimVocoder
    from kokoro_ruslan_amd.spec import ModelDims, StepHyper
    d, P = _fixture()
    e = KokoroEngine(ModelDims(**d.__dict__), StepHyper(), math_mode="f32", init=False, total_steps=100)
    e.load_params(P)
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(1, d.vocab, (n,), generator=g).cuda() for n in PHONEMES]
    st = [torch.randint(0, 3, (n,), generator=g).cuda() for n in PHONEMES]
    mels, info = e.generate_stream(ids, st, slots=2, want_info=True, **STOP_AT_MIN)      # computed once, never changed
    voc, ex = GriffinLimVocoder(), FeatureExtractor()
    own = ex.extract(vocode(voc, mels, **_gl()), max_seq_length=4097)                     # the engine's own mels as audio, as tracks
    # references a fifth longer than the mels: warped noisy copies with random tracks
    refs, ref_pitch, ref_energy = [], [], []
    for m in mels:
        idx = torch.linspace(0, m.shape[0] - 1, int(1.2 * m.shape[0]) + 1).round().long()
        refs.append(m.cpu()[idx] + 0.05 * torch.randn(idx.numel(), m.shape[1], generator=g))
        ref_pitch.append(pitch_track(g, idx.numel()))
        ref_energy.append(torch.rand(idx.numel(), generator=g))
    return dict(e=e, ids=ids, st=st, mels=mels, info=info, voc=voc, ex=ex, own=own, refs=refs, ref_pitch=ref_pitch,
                ref_energy=ref_energy, al=MelAligner())


def _check_against_the_oracle(w, recs, audio, mels):
    """Every new field of the records is the oracle's on the tracks of `audio` (extracted here) along the device's path."""
    feats = w["ex"].extract(audio, max_seq_length=4097)
    paths = w["al"].align(mels, w["refs"], want_path=True)
    for i, (r, f, al, m) in enumerate(zip(recs, feats, paths, mels)):
        T = m.shape[0]
        assert audio[i].numel() == 256 * (T - 1) and f["pitch"].numel() == T == r["frames"]
        path = al["path"].cpu().numpy()
        want = R.track_metrics(R.track_stats(path, f["pitch"][:T], w["ref_pitch"][i], f["energy"][:T], w["ref_energy"][i]), len(path))
        print(f"utterance {i}: {T} frames, {len(path)} steps  " + "  ".join(f"{k} {r[k]!r} / {want[k]!r}" for k in TRACK_KEYS))
        assert r["no_variance"] is False
        for k in ("n_vv", "n_vu", "n_uv", "n_uu", "n_gpe", "gpe", "vuv_err"):
            assert r[k] == want[k], (i, k)
        assert close(r["energy_l1_dtw"] * len(path), want["energy_l1_dtw"] * len(path))
        if want["n_vv"]:
            n = want["n_vv"]
            assert close(r["f0_bias_cents"] * n, want["f0_bias_cents"] * n) and close(r["f0_rmse_cents"] ** 2 * n, want["f0_rmse_cents"] ** 2 * n)
        else:
            assert r["f0_bias_cents"] is None and r["f0_rmse_cents"] is None


def test_every_new_field_is_the_oracles_on_the_returned_audio(world):
    from kokoro.inference.evaluate import evaluate
    w = world
    recs, summ, audio = evaluate(w["e"], w["ids"], w["st"], w["refs"], slots=2, vocoder=w["voc"], vocoder_kwargs=_gl(), extractor=w["ex"],
                                 ref_pitch=w["ref_pitch"], ref_energy=w["ref_energy"], want_audio=True, **STOP_AT_MIN)
    assert len(audio) == 4 and all(a.is_cuda and a.dim() == 1 for a in audio)
    _check_against_the_oracle(w, recs, audio, w["mels"])
    assert summ["no_variance"] == 0 and "vuv_err" in summ and "energy_l1_dtw" in summ
    assert sum(r["n_vu"] + r["n_uv"] + r["n_uu"] for r in recs) > 0, "the references have unvoiced runs"


def test_stream_and_batches_give_the_same_records(world):
    """generate_stream documents its mels within 1e-4 of generate_batch's, not bit for bit, so "the same" carries bounds, stated here
    before anything is measured (the figures are printed):
      mel side      as test_evaluate_gpu.py: mel_l1_dtw within 1e-4, mcd_dtw within (10 / ln 10) sqrt(2) sqrt(M) 1e-4.
      audio         relative L2 of the two paths' waveforms <= 1e-2: 1e-4 in a log-mel is 1e-4 relative in power, and four Griffin-Lim
                    iterations from the same phases magnify an input perturbation by a few tens (DESIGN (f)7: fp32 rounding, 1.2e-7,
                    comes out as 8.5e-7 to 4.6e-6 at 4 iterations: x40), so about 4e-3.  This is the check that both paths hand the
                    vocoder the same content.
      counts        each of n_vv, n_vu, n_uv, n_uu, n_gpe differs by at most 6 steps, vuv_err by at most 6 / steps: a perturbation
                    of that size can flip a voicing decision only on a frame that sits on its threshold; one such flip is spread by
                    the tracker's gap fill over at most MAX_GAP = 5 frames, and the path may visit a frame more than once.
      energy        energy_l1_dtw within 0.05: the normalised energy lives in [0, 1] and five hundredths of that range is the
                    resolution of interest of the metric, more than two orders above the 1e-4 of the mels.
      F0            where no count differs and n_vv >= 8: f0_rmse_cents and f0_bias_cents within 5 cents (the bound and the argument
                    of the whole-tone run below: the resolution of interest is tens of cents), gpe equal (it is n_gpe / n_vv).
    Each path's records are also the oracle's on that path's own mels and audio."""
    import math
    from kokoro.inference.evaluate import _generate, evaluate
    w = world
    kw = dict(vocoder=w["voc"], extractor=w["ex"], ref_pitch=w["ref_pitch"], ref_energy=w["ref_energy"], want_audio=True, **STOP_AT_MIN)
    a, sa, wa = evaluate(w["e"], w["ids"], w["st"], w["refs"], stream=True, slots=2, vocoder_kwargs=_gl(), **kw)
    b, sb, wb = evaluate(w["e"], w["ids"], w["st"], w["refs"], stream=False, batch_size=3, vocoder_kwargs=_gl(), **kw)
    batch_mels, _ = _generate(w["e"], w["ids"], w["st"], False, 0, 3, STOP_AT_MIN)        # the mels of evaluate()'s batch path
    _check_against_the_oracle(w, a, wa, w["mels"])
    _check_against_the_oracle(w, b, wb, batch_mels)
    assert [list(x) for x in a] == [list(y) for y in b] and set(sa) == set(sb)
    M = w["mels"][0].shape[1]
    COUNTS = ("n_vv", "n_vu", "n_uv", "n_uu", "n_gpe")
    for i, (x, y, u, v) in enumerate(zip(a, b, wa, wb)):
        assert {k: x[k] for k in ("name", "frames", "ref_frames", "len_ratio", "hit_bound", "no_variance")} == \
               {k: y[k] for k in ("name", "frames", "ref_frames", "len_ratio", "hit_bound", "no_variance")}
        steps = x["n_vv"] + x["n_vu"] + x["n_uv"] + x["n_uu"]
        rel = float((u.double() - v.double()).norm() / u.double().norm())
        print(f"utterance {i}: {steps} steps  audio relative L2 {rel:.3e}  mcd_dtw {x['mcd_dtw']!r} / {y['mcd_dtw']!r}  " +
              "  ".join(f"{k} {x[k]!r} / {y[k]!r}" for k in TRACK_KEYS))
        assert steps >= max(x["frames"], x["ref_frames"]) and steps == y["n_vv"] + y["n_vu"] + y["n_uv"] + y["n_uu"]
        assert abs(x["mel_l1_dtw"] - y["mel_l1_dtw"]) <= 1e-4
        assert abs(x["mcd_dtw"] - y["mcd_dtw"]) <= 10 / math.log(10) * math.sqrt(2) * math.sqrt(M) * 1e-4
        assert u.shape == v.shape and rel <= 1e-2
        for k in COUNTS:
            assert abs(x[k] - y[k]) <= 6, (i, k)
        assert abs(x["vuv_err"] - y["vuv_err"]) <= 6 / steps
        assert abs(x["energy_l1_dtw"] - y["energy_l1_dtw"]) <= 0.05
        if all(x[k] == y[k] for k in COUNTS) and x["n_vv"] >= 8:
            assert abs(x["f0_rmse_cents"] - y["f0_rmse_cents"]) <= 5.0 and abs(x["f0_bias_cents"] - y["f0_bias_cents"]) <= 5.0
            assert x["gpe"] == y["gpe"]
    assert sum(x["n_vv"] >= 8 for x in a) >= 2, "the F0 bound is exercised"
    assert sa["utterances"] == sb["utterances"] == 4 and sa["no_variance"] == sb["no_variance"] == 0


def test_against_its_own_audio_the_track_errors_are_zero(world):
    from kokoro.inference.evaluate import evaluate
    w = world
    T = [m.shape[0] for m in w["mels"]]
    recs, summ = evaluate(w["e"], w["ids"], w["st"], w["mels"], slots=2, vocoder=w["voc"], vocoder_kwargs=_gl(), extractor=w["ex"],
                          ref_pitch=[f["pitch"][:t] for f, t in zip(w["own"], T)], ref_energy=[f["energy"][:t] for f, t in zip(w["own"], T)],
                          **STOP_AT_MIN)
    for r, f, t in zip(recs, w["own"], T):
        voiced = int((f["pitch"][:t] > 0).sum())
        print(f"{t} frames, {voiced} voiced: " + "  ".join(f"{k} {r[k]!r}" for k in TRACK_KEYS))
        assert r["mcd_dtw"] == 0.0 and r["vuv_err"] == 0.0 and r["energy_l1_dtw"] == 0.0
        assert r["n_vv"] == voiced and r["n_uu"] == t - voiced and r["n_vu"] == r["n_uv"] == r["n_gpe"] == 0
        if voiced:
            assert r["f0_rmse_cents"] == 0.0 and r["f0_bias_cents"] == 0.0 and r["gpe"] == 0.0
        else:
            assert r["f0_rmse_cents"] is None and r["gpe"] is None
    assert sum(r["n_vv"] for r in recs) > 0, "some frame of the four utterances is voiced"
    assert summ["vuv_err"] == {"mean": 0.0, "median": 0.0, "p95": 0.0} and summ["f0_rmse_cents"]["mean"] == 0.0


def test_without_a_vocoder_the_records_are_the_parents(world):
    from kokoro.inference.evaluate import evaluate
    w = world
    durs = [d + 1 for d in w["info"]["durations"]]
    old = evaluate(w["e"], w["ids"], w["st"], w["refs"], slots=2, durations=durs, names=list("abcd"), **STOP_AT_MIN)
    new = evaluate(w["e"], w["ids"], w["st"], w["refs"], slots=2, durations=durs, names=list("abcd"), vocoder=None, vocoder_kwargs=None,
                   denoiser=None, denoise_strength=0.005, extractor=None, ref_pitch=None, ref_energy=None, want_audio=False, **STOP_AT_MIN)
    assert new == old and len(new) == 2
    assert all(set(r) == {"name", "frames", "ref_frames", "len_ratio", "mcd_dtw", "mel_l1_dtw", "hit_bound", "dur_abs_err"} for r in new[0])
    assert set(new[1]) == {"utterances", "hit_bound_share", "mcd_dtw", "mel_l1_dtw", "len_ratio", "dur_abs_err"}


def test_kokoro_eval_griffin_lim_reports_the_new_metrics(tmp_path, capsys):
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
    cache = tmp_path / "cache"
    cache.mkdir()
    g = torch.Generator().manual_seed(4)
    for i, (P, T) in enumerate([(5, 20), (9, 31), (7, 26)]):
        dur = torch.ones(P, dtype=torch.int64)
        dur[-1] = T - (P - 1)
        bare = i == 1                                                                 # the middle utterance: written without variance
        torch.save({"mel_spec": torch.randn(80, T, generator=g) - 5.0, "phoneme_indices": torch.randint(1, 59, (P,), generator=g),
                    "stress_indices": torch.zeros(P, dtype=torch.int64), "phoneme_durations": dur, "stop_token_targets": torch.zeros(T),
                    "pitch": torch.zeros(T) if bare else pitch_track(g, T), "energy": torch.zeros(T) if bare else torch.rand(T, generator=g),
                    "mel_length": T, "phoneme_length": P, "text": "", "audio_file": f"u{i}.wav", "_cache_version": FEATURE_CACHE_VERSION},
                   cache / f"u{i}.pt")
    base = ["--checkpoint", str(ck), "--features", str(cache), "--split", "all", "--math", "f32", "--weights", "model", "--max-len", "40",
            "--min-len-floor", "8", "--slots", "2"]
    plain, audio = tmp_path / "plain.json", tmp_path / "audio.json"
    assert cli.main(base + ["--output", str(plain)]) == 0
    out_plain = capsys.readouterr().out
    assert cli.main(base + ["--output", str(audio), "--griffin-lim", "--griffin-lim-iters", "4", "--griffin-lim-seed", "3", "--gpe-ratio", "0.1"]) == 0
    out_audio = capsys.readouterr().out
    rp, ra = json.loads(plain.read_text()), json.loads(audio.read_text())
    assert [r["name"] for r in ra["records"]] == [r["name"] for r in rp["records"]] == ["u0", "u2", "u1"]      # (length-sorted)
    for r in rp["records"]:
        assert not set(r) & (set(TRACK_KEYS) | {"no_variance"})
    assert not set(rp["summary"]) & (set(TRACK_KEYS) | {"no_variance"}) and "audio" not in rp and "gpe_ratio" not in rp
    assert not any(k in out_plain for k in ("f0_rmse_cents", "vuv_err", "audio:"))
    for r, q in zip(ra["records"], rp["records"]):
        assert {k: r[k] for k in q} == q, "the mel side of the report is the same"
        if r["name"] == "u1":
            assert r["no_variance"] is True and not set(r) & set(TRACK_KEYS)
        else:
            assert r["no_variance"] is False and set(TRACK_KEYS) <= set(r) and 0.0 <= r["vuv_err"] <= 1.0 and r["energy_l1_dtw"] >= 0.0
            assert r["n_vv"] + r["n_vu"] + r["n_uv"] + r["n_uu"] >= max(r["frames"], r["ref_frames"])
    assert ra["summary"]["no_variance"] == 1 and {"vuv_err", "energy_l1_dtw"} <= set(ra["summary"])
    assert ra["gpe_ratio"] == 0.1 and ra["audio"] == "Griffin-Lim, 4 iterations"
    lines = out_audio.splitlines()
    assert "audio: Griffin-Lim, 4 iterations, 1 without pitch and energy in the cache" in lines[0]
    assert {"vuv_err", "energy_l1_dtw"} <= {ln.split()[0] for ln in lines[1:]}
    assert out_plain.splitlines()[1:5] == lines[1:5], "the four mel metrics print as they always did"


# ---- one sanity run on real signal ------------------------------------------------------------------------------------------------

def test_a_whole_tone_apart_reads_two_hundred_cents():
    """Two synthetic harmonic waveforms (features_torch.test_signal, 4 s, seeds 0 and 1), the synthesized side at the reference's F0
    x 2^(2/12), through FeatureExtractor and align(tracks=) on their own mels.  The fp64 pipeline (features_torch.extract in fp64,
    dtw_torch.dtw on its mels, dtw_torch.track_stats) gives on these two waveforms f0_bias_cents = 200.3832 (f0_rmse_cents 200.43,
    gpe 0, 189 of 354 steps voiced on both sides): not 200 by construction (the tracker's parabolic interpolation, the voicing
    edges).  The device's value is held to that +- 5 cents: the metric's resolution of interest is tens of cents, and the few frames
    whose voicing differs between fp32 and fp64 move a mean over some 190 voiced frames by far less."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro_ruslan_amd import features_torch as FT
    from kokoro_ruslan_amd.dtw import MelAligner
    from kokoro_ruslan_amd.features import FeatureExtractor
    FP64_BIAS = 200.3832
    lo, hi = FT.test_signal(88200, seed=0, f0=120.0), FT.test_signal(88200, seed=1, f0=120.0 * 2.0 ** (2.0 / 12.0))
    fa, fb = FeatureExtractor().extract([hi.float(), lo.float()], max_seq_length=4097)
    rec = MelAligner().align([fa["mel_spec"].t().contiguous()], [fb["mel_spec"].t().contiguous()],
                             tracks={"pitch": ([fa["pitch"]], [fb["pitch"]]), "energy": ([fa["energy"]], [fb["energy"]])})[0]
    print({k: rec[k] for k in TRACK_KEYS}, rec["steps"])
    assert rec["n_vv"] >= 100, "the mean runs over hundreds of voiced steps: what the bound's argument rests on"
    assert abs(rec["f0_bias_cents"] - FP64_BIAS) <= 5.0
