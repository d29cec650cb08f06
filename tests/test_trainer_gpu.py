"""GPU suite: `kokoro-train` end to end on a synthetic feature cache — epochs, validation on the EMA weights,
checkpoints in the reference layout, strict resume."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

REF_CKPT_KEYS = {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict",
                 "current_optimizer_step", "optimizer_steps_completed", "loss", "train_loss", "val_loss", "val_mel_loss",
                 "val_stop_loss", "val_dur_loss", "best_val_loss", "best_val_epoch", "config", "model_metadata",
                 "scheduler_config", "ema_model_state_dict", "ema_updates"}


def _fake_cache(root, n=12, tmin=40, tmax=120, pmin=4, pmax=14, extra_frames=()):
    """n synthetic utterances in the reference's cache schema (v7); utterance i of `extra_frames` gets that many frames
    added to one phoneme's duration, so its durations expand beyond its mel length (a clipped utterance)."""
    from kokoro_ruslan_amd.synthetic import synthetic_batch
    d = root / ".feature_cache"
    d.mkdir(parents=True)
    g = torch.Generator().manual_seed(0)
    for i in range(n):
        T = tmin if tmin == tmax else int(torch.randint(tmin, tmax, (1,), generator=g))
        P = pmin if pmin == pmax else int(torch.randint(pmin, pmax, (1,), generator=g))
        b = synthetic_batch(1, T, P, seed=i)
        if i < len(extra_frames):
            b["phoneme_durations"][0, P // 2] += extra_frames[i]
        torch.save({"mel_spec": b["mel_specs"][0].T.contiguous(), "phoneme_indices": b["phoneme_indices"][0],
                    "stress_indices": b["stress_indices"][0], "phoneme_durations": b["phoneme_durations"][0],
                    "stop_token_targets": b["stop_token_targets"][0], "pitch": b["pitches"][0], "energy": b["energies"][0],
                    "text": f"utt {i}", "audio_file": f"utt{i:03d}", "mel_length": T, "phoneme_length": P,
                    "_cache_version": 7}, d / f"utt{i:03d}.pt")


@pytest.mark.parametrize("strict_guard", [False, True])
def test_kokoro_train_cli_end_to_end(tmp_path, monkeypatch, strict_guard):
    """strict_guard: the per-micro-batch host check (KK_STRICT_NONFINITE=1), which drives the engine's micro_batch / finish_cycle
    itself instead of train_step_auto; everything below holds for both."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    monkeypatch.setenv("KK_STRICT_NONFINITE", "1" if strict_guard else "0")
    from kokoro.cli.training import main
    from kokoro.training import checkpoint as ckpt
    from kokoro_ruslan_amd import spec
    corpus, out = tmp_path / "corpus", tmp_path / "model"
    _fake_cache(corpus)
    args = ["--corpus", str(corpus), "--output", str(out), "--no-mfa", "--no-dynamic-batching", "--batch-size", "4",
            "--epochs", "2", "--save-every", "1", "--val-split", "0.25"]
    assert main(args) == 0
    files = sorted(os.listdir(out))
    assert "checkpoint_epoch_1.pth" in files and "checkpoint_epoch_2.pth" in files and "kokoro_russian_final.pth" in files
    c = torch.load(out / "checkpoint_epoch_2.pth", map_location="cpu", weights_only=False)
    assert REF_CKPT_KEYS <= set(c.keys())
    assert list(c["model_state_dict"].keys()) == spec.state_dict_order(spec.ModelDims())
    assert type(c["config"]).__module__ == "kokoro.training.config"
    arch = c["model_metadata"]["architecture"]
    assert c["model_metadata"]["schema_version"] == 2 and arch["hidden_dim"] == 512 and arch["vocab_size"] == 59
    osd = c["optimizer_state_dict"]
    assert [g["group_type"] for g in osd["param_groups"]] == list(spec.GROUP_TYPES)
    assert sum(len(g["params"]) for g in osd["param_groups"]) == 308 and len(osd["state"]) == 308
    steps = c["optimizer_steps_completed"]
    assert steps == 4                                        # 9 train utts / batch 4 = 3 batches, G=2 -> 2 steps/epoch
    assert c["val_loss"] is not None and c["val_loss"] == c["val_loss"]          # finite number
    fin = torch.load(out / "kokoro_russian_final.pth", map_location="cpu", weights_only=False)
    assert set(fin.keys()) == {"model_state_dict", "config", "model_metadata"}
    # EMA differs from the live weights after training and both are finite
    w, e = c["model_state_dict"]["decoder.layers.0.ff.linear1.weight"], c["ema_model_state_dict"]["decoder.layers.0.ff.linear1.weight"]
    assert torch.isfinite(w).all() and torch.isfinite(e).all() and not torch.equal(w, e)
    # strict resume: a third epoch continues from the saved optimizer-step counter
    assert main(args[:-6] + ["--epochs", "3", "--save-every", "1", "--val-split", "0.25", "--resume", "auto"]) == 0
    c3 = torch.load(out / "checkpoint_epoch_3.pth", map_location="cpu", weights_only=False)
    assert c3["optimizer_steps_completed"] == steps + 2 and c3["epoch"] == 2
    # architecture mismatch is refused like the reference's strict loader
    from kokoro_ruslan_amd.engine import KokoroEngine
    small = KokoroEngine(spec.ModelDims(hidden=128, heads=2, enc_layers=1, dec_layers=1, enc_ff=96, dec_ff=96, var_filter=32,
                                        var_bins=16, mel=80, max_len=4000), spec.StepHyper())
    with pytest.raises(RuntimeError, match="architecture mismatch"):
        ckpt.load_checkpoint(small, str(out / "checkpoint_epoch_3.pth"))


def test_validation_metrics_match_per_sample_loops(tmp_path):
    """validate_epoch's masked, on-device spectral convergence / F0-RMSE == the reference's per-sample Python loops
    (trainer.py:1866-1910) on the same predictions."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import math
    from kokoro.cli.cli import create_config_from_args, parse_arguments
    from kokoro.data.cached import collate_fn
    from kokoro.training.trainer import KokoroTrainer, cap_batch
    corpus = tmp_path / "corpus"
    _fake_cache(corpus, n=14)
    import sys
    argv, sys.argv = sys.argv, ["kokoro-train", "--corpus", str(corpus), "--output", str(tmp_path / "m"), "--no-mfa",
                                "--no-dynamic-batching", "--batch-size", "3", "--epochs", "1", "--val-split", "0.4"]
    try:
        cfg = create_config_from_args(parse_arguments())
    finally:
        sys.argv = argv
    tr = KokoroTrainer(cfg)
    val = tr.validate_epoch()
    e = tr.engine
    sc_sum = sc_n = f0_sum = f0_n = 0.0
    with e.fp32_math(), e.ema_weights():
        for idxs in tr._val_batches():
            batch = cap_batch(tr._to_device(collate_fn([tr.val_dataset[j] for j in idxs])))
            out = e.forward_backward(batch, backward=False)
            bs = bn = fs = fn = 0.0
            for b in range(batch["mel_specs"].size(0)):
                L = int(batch["mel_lengths"][b])
                ref, pred = batch["mel_specs"][b, :L], out["mel"][b, :L]
                den = float(torch.norm(ref))
                if den > 0:
                    bs += float(torch.norm(ref - pred)) / den
                    bn += 1
                fs += math.sqrt(float(torch.mean((batch["pitches"][b, :L] - out["pitch"][b, :L]) ** 2)))
                fn += 1
            sc_sum, sc_n, f0_sum, f0_n = sc_sum + bs / bn, sc_n + 1, f0_sum + fs / fn, f0_n + 1
    assert abs(val["spectral_convergence"] - sc_sum / sc_n) < 1e-5 * max(1.0, sc_sum / sc_n)
    assert abs(val["f0_rmse"] - f0_sum / f0_n) < 1e-5
    assert len(tr._val_batches()) >= 2 and sorted(i for b in tr._val_batches() for i in b) == list(range(len(tr.val_dataset)))


def _config(tmp_path, corpus, *flags):
    import sys
    from kokoro.cli.cli import create_config_from_args, parse_arguments
    argv, sys.argv = sys.argv, ["kokoro-train", "--corpus", str(corpus), "--output", str(tmp_path / "m"), "--no-mfa", *flags]
    try:
        return create_config_from_args(parse_arguments())
    finally:
        sys.argv = argv


def test_trainer_turns_regularisation_on_and_validation_off(tmp_path):
    """kokoro-train trains with the configured dropout / stochastic depth / SpecAugment (reference model.train(),
    trainer.py:2038-2056) and validates without: an epoch over the same data twice gives different losses, validation
    twice gives the same, and a failure inside validation leaves the live weights and flags untouched."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.training.trainer import KokoroTrainer
    corpus = tmp_path / "corpus"
    _fake_cache(corpus, n=10)
    cfg = _config(tmp_path, corpus, "--no-dynamic-batching", "--batch-size", "4", "--epochs", "2", "--val-split", "0.3")
    cfg.learning_rate = 0.0                                  # the weights stay put: only the masks can change the loss
    cfg.spec_augment_start_epoch = 1
    tr = KokoroTrainer(cfg)
    e = tr.engine
    seen = []
    orig = e.train_step_auto

    def spy(*a, **k):
        seen.append((e.train_dropout, e.spec_augment_active))
        return orig(*a, **k)
    e.train_step_auto = spy
    l0 = tr.train_epoch(0)
    assert seen and all(s == (True, False) for s in seen)    # epoch 0 < spec_augment_start_epoch
    n0 = len(seen)
    tr.sampler.epoch = 0
    batches0 = tr.sampler.batches()
    l1 = tr.train_epoch(0)
    assert tr.sampler.batches() == batches0 and l0 != l1, "same batches, same weights: only fresh dropout masks differ"
    tr.train_epoch(1)
    assert all(s == (True, True) for s in seen[2 * n0:])
    assert e.train_dropout is False
    v0, v1 = tr.validate_epoch(), tr.validate_epoch()
    assert v0["total"] == v1["total"] and v0["total"] == v0["total"]
    # an exception inside validation must not leave the EMA slab as the live weights
    p_before, P_before, math_before = e.arena.p.data_ptr(), e.arena.P, e.math
    boom = e.forward_backward
    e.forward_backward = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        tr.validate_epoch()
    e.forward_backward = boom
    assert e.arena.p.data_ptr() == p_before and e.arena.P is P_before and e.math == math_before and e.train_dropout is False


def test_dynamic_batching_200_steps_memory_flat(tmp_path):
    """BASELINE configs[2] on a synthetic ragged cache: dynamic batching with --max-frames 16384 (B in [4, 32], a new
    batch shape nearly every step), MFA-style durations baked into the cache with some utterances whose durations expand
    beyond their mel length.  >= 200 optimizer micro-steps with all regularisation on: finite losses, no skipped
    optimizer step, device memory flat after the first epoch."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.training.trainer import KokoroTrainer
    corpus = tmp_path / "corpus"
    _fake_cache(corpus, n=1200, tmin=90, tmax=1500, pmin=12, pmax=60, extra_frames=[3, 1, 7, 2, 5, 4, 9, 1, 2, 6] * 8)
    cfg = _config(tmp_path, corpus, "--max-frames", "16384", "--min-batch-size", "4", "--max-batch-size", "32", "--epochs", "2",
                  "--val-split", "0.05")
    cfg.use_mixed_precision, cfg.mixed_precision_dtype = True, "bfloat16"
    assert cfg.use_dynamic_batching
    tr = KokoroTrainer(cfg)
    e = tr.engine
    shapes, expanded = set(), 0
    orig = e.train_step_auto

    def spy(batch, *a, **k):
        nonlocal expanded
        shapes.add((tuple(batch["mel_specs"].shape[:2]), batch["phoneme_indices"].shape[1]))
        expanded += a[3] is not None if len(a) > 3 else k.get("expanded_len") is not None
        return orig(batch, *a, **k)
    e.train_step_auto = spy
    l0 = tr.train_epoch(0)
    torch.cuda.synchronize()
    n_epoch = len(tr.sampler)
    mem0, ws0 = torch.cuda.memory_allocated(), e.workspace_bytes()
    l1 = tr.train_epoch(1)
    l2 = tr.train_epoch(2)
    torch.cuda.synchronize()
    mem1, ws1 = torch.cuda.memory_allocated(), e.workspace_bytes()
    st = e.opt_stats()
    assert 3 * n_epoch >= 200 and len(shapes) >= 40, (n_epoch, len(shapes))
    assert expanded >= 5, "some batches must have carried durations that expand beyond the mel length"
    assert all(x == x and abs(x) < 1e4 for x in (l0, l1, l2))
    assert st["skipped"] == 0 and st["attempt"] >= 100
    assert bool(torch.isfinite(e.arena.p).all())
    assert ws1 <= ws0 * 1.15 and mem1 <= mem0 * 1.15 + (64 << 20), (ws0, ws1, mem0, mem1)
    assert max(b * t for (b, t), _ in shapes) <= 16384
    val = tr.validate_epoch()
    assert val is not None and val["total"] == val["total"]


def test_kokoro_train_reaches_bench_speed_on_a_fixed_shape(tmp_path):
    """The path that actually trains (kokoro-train: loader thread + pinned staging + graph replay with the reference's
    default accumulation G = 2) against bench.py's loop (resident batch, train_step_graphed, G = 1) at the same shape:
    frames/s within 15 % once the graphs exist (the trainer also pays an optimizer pass only every second micro-batch,
    so it is compared against the bench loop run with G = 2 as well)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import time
    from kokoro.training.trainer import KokoroTrainer
    from kokoro_ruslan_amd.synthetic import synthetic_batch
    corpus = tmp_path / "corpus"
    _fake_cache(corpus, n=8 * 40, tmin=512, tmax=512, pmin=64, pmax=64)
    cfg = _config(tmp_path, corpus, "--no-dynamic-batching", "--batch-size", "8", "--epochs", "4", "--val-split", "0.0")
    cfg.use_mixed_precision, cfg.mixed_precision_dtype = True, "bfloat16"
    tr = KokoroTrainer(cfg)
    e = tr.engine
    assert len(tr.sampler) == 40
    tr.train_epoch(0)                                        # shapes seen, graphs captured, files in the page cache
    tr.train_epoch(1)                                        # (SpecAugment switches on at epoch 1: one more capture)
    dt_train = float("inf")
    for ep in (2, 3):                                        # best of two epochs: a host-side hiccup of the box (page cache, a
        torch.cuda.synchronize()                             # neighbour's burst) in one 0.15 s epoch is not what this test is about
        t0 = time.perf_counter()
        tr.train_epoch(ep)                                   # (ends with the epoch's one host read)
        dt_train = min(dt_train, time.perf_counter() - t0)
    print(f"loader: {tr.last_prefetch.load_s / 40 * 1e3:.2f} ms per batch on its thread, {tr.last_prefetch.wait_s / 40 * 1e3:.2f} ms waiting for the GPU; "
          f"epoch {dt_train * 1e3:.1f} ms")
    fps_train = 40 * 8 * 512 / dt_train
    b = {k: v.cuda() for k, v in synthetic_batch(8, 512, 64, seed=1).items()}
    e.train_dropout = True
    e.micro_in_cycle = 0
    for _ in range(6):
        e.train_step_graphed(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(40):
        e.train_step_graphed(b)
    torch.cuda.synchronize()
    fps_bench = 40 * 8 * 512 / (time.perf_counter() - t0)
    print(f"kokoro-train {fps_train:,.0f} frames/s, resident-batch loop {fps_bench:,.0f} frames/s (G = 2)")
    assert fps_train >= 0.85 * fps_bench, (fps_train, fps_bench)
    assert e.opt_stats()["skipped"] == 0


def test_trainer_legacy_schedule_and_ema_cadence(tmp_path):
    """TrainingConfig.use_onecycle_lr = False and ema_update_every = 2 through kokoro-train's trainer (both were refused before round 5):
    every optimizer step of epoch e runs at the CosineAnnealingWarmRestarts value after e scheduler steps (reference trainer.py:789-799,
    2885-2887) — also through the replayed optimizer graphs, which are re-captured when the epoch's factor changes — the EMA moves on every
    second successful step, and the checkpoint carries a scheduler state torch's own class continues from."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from kokoro.training import checkpoint as ckpt
    from kokoro.training.trainer import KokoroTrainer
    from kokoro_ruslan_amd import spec
    corpus = tmp_path / "corpus"
    _fake_cache(corpus, n=16, tmin=64, tmax=64, pmin=8, pmax=8)          # one batch shape: the second step of it is a graph replay
    cfg = _config(tmp_path, corpus, "--no-dynamic-batching", "--batch-size", "4", "--epochs", "4", "--val-split", "0.0")
    cfg.use_onecycle_lr, cfg.lr_T_0, cfg.lr_T_mult, cfg.lr_eta_min = False, 2, 2, 1e-6
    cfg.ema_update_every, cfg.ema_decay, cfg.gradient_accumulation_steps = 2, 0.9, 1
    tr = KokoroTrainer(cfg)
    e = tr.engine
    assert e.hp.use_onecycle_lr is False and e.hp.ema_update_every == 2
    lrs, moved = [], []
    orig = e.train_step_auto

    def spy(*a, **k):
        before = e.arena.ema.clone()
        out = orig(*a, **k)
        torch.cuda.synchronize()
        lrs.append((e.lr_epoch, e.opt_stats()["last_base_lr"]))
        moved.append(not torch.equal(e.arena.ema, before))
        return out
    e.train_step_auto = spy
    for epoch in range(3):
        tr.train_epoch(epoch)
    assert len(lrs) == 12 and all(ep == i // 4 for i, (ep, _) in enumerate(lrs))
    for ep, lr in lrs:
        want = cfg.lr_eta_min + (cfg.learning_rate - cfg.lr_eta_min) * spec.cosine_restart_factor(ep, 2, 2)
        assert abs(lr - want) <= 1e-12, (ep, lr, want)
    assert lrs[0][1] == lrs[8][1] and lrs[4][1] < 0.6 * lrs[0][1]      # epoch 2 is a restart (T_0 = 2), epoch 1 the half-way point
    assert moved == [i % 2 == 0 for i in range(12)]                     # successful steps 0, 2, 4, ...
    path = ckpt.save_checkpoint(e, cfg, 2, 1.0, str(tmp_path / "out"))
    c = torch.load(path, map_location="cpu", weights_only=False)
    mults = [m for m, _ in spec.group_lr_mult_wd(e.hp)]
    opt = torch.optim.AdamW([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": cfg.learning_rate * m} for m in mults])
    sch = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2, eta_min=1e-6)
    for g, s in zip(opt.param_groups, c["optimizer_state_dict"]["param_groups"]):
        g["lr"], g["initial_lr"] = s["lr"], s["initial_lr"]
    sch.load_state_dict(c["scheduler_state_dict"])
    f3, f4 = spec.cosine_restart_factor(3, 2, 2), spec.cosine_restart_factor(4, 2, 2)
    for g, m in zip(opt.param_groups, mults):                            # the groups carry the NEXT epoch's lr (the reference steps before it saves)
        assert abs(g["lr"] - (cfg.lr_eta_min + (cfg.learning_rate * m - cfg.lr_eta_min) * f3)) <= 1e-15 + 1e-12 * g["lr"]
    opt.step()
    sch.step()
    for g, m in zip(opt.param_groups, mults):
        assert abs(g["lr"] - (cfg.lr_eta_min + (cfg.learning_rate * m - cfg.lr_eta_min) * f4)) <= 1e-15 + 1e-12 * g["lr"]
