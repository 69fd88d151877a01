"""Checks of the ``streaming_validation`` option of train.train (streaming.StreamingValidation, streaming.validate_streaming),
shared by the emulator tests (tests/test_streaming_validation_emulated.py) and the GPU test
(tests/test_streaming_validation_gpu.py).  The loop is the tiny run of tests/stream_mine_checks.py (12 steps, boundaries at 4, 8
and 12); every comparison is exact: the logged metrics against ``streaming.operating_summary_host`` +
``streaming.select_operating_points`` on the probabilities read back at the same weights, weights and logs byte for byte."""
import glob
import json
import math
import os
import random

import numpy as np
import pytest

from microwakeword_amd import streaming
from microwakeword_amd import train as tr
from microwakeword_amd.data import FeatureHandler
import engine_checks as ec
import mining_checks as mc
import stream_mine_checks as smc

SV = dict(target_faph=0.5, windows=[5, 3])
BOUNDARIES = [4, 8, 12]
STREAMING_NAMES = dict(minimization_metric="streaming_false_accepts_per_hour", maximization_metric="streaming_cutoff", target_minimization=0.5)


def config(tmp_path, name, sv=None, mining_map=None, **over):
    cfg = smc.loop_config(tmp_path, name, mining_map)
    if sv is not None:
        cfg["streaming_validation"] = dict(sv)
    cfg.update(over)
    return cfg


def log_of(cfg, which):
    with open(os.path.join(cfg["summaries_dir"], which, "scalars.jsonl")) as fh:
        return [json.loads(line) for line in fh]


def log_bytes(cfg, which):
    with open(os.path.join(cfg["summaries_dir"], which, "scalars.jsonl"), "rb") as fh:
        return fh.read()


def weights_at(cfg, step):
    """the weights file the run saved at a boundary (the last step's: last_weights)"""
    if step == smc.STEPS:
        return os.path.join(cfg["train_dir"], "last_weights.weights.h5")
    found = glob.glob(os.path.join(cfg["train_dir"], "train", "*_weights_%d.weights.h5*" % step))
    assert len(found) == 1, found
    return found[0].replace(".npz", "")


def file_arrays(path):
    with np.load(path + ".npz") as z:
        return {k: z[k].tobytes() for k in z.files}


def restated(lib, cfg, weights=None):
    """the streaming metrics of a fresh model (the run's initial weights, or a weights file of the run) by the host
    restatement on the probabilities read back"""
    from microwakeword_amd import mixednet
    v = streaming.streaming_validation_config(cfg)
    random.seed(1)
    np.random.seed(1)
    fresh = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    if weights is not None:
        fresh.load_weights(weights)
    fh = FeatureHandler(cfg, engine=fresh.engine)
    sm = streaming.StreamingModel(fresh, int(cfg["stride"]), v["mode"])
    amb, _ = fh.track_windows(v["ambient_set"], sm.frames)
    pos, _ = fh.track_windows(v["data_set"], sm.frames, only_label=1.0)
    sm.reset()
    off = sm.native.run(np.concatenate([amb, pos]))
    p = sm.read_probabilities()
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    host = streaming.operating_summary_host(tracks[:amb.size], tracks[amb.size:], v["windows"], streaming.CUTOFFS, sm.stride,
                                            cfg["window_step_ms"] / 1000, v["ignore_slices_after_accept"], v["target_faph"])
    return streaming.streaming_metrics(host), host


def same_metrics(line, metrics, step):
    assert set(line) == set(streaming.STREAMING_METRICS) | {"step"} and line["step"] == step, line
    for k, want in metrics.items():
        got, want = line[k], float(want)
        assert got == want or (math.isnan(got) and math.isnan(want)), (step, k, got, want)
    return True


def check_restatement(lib, tmp_path, sv=SV):
    """the line logged at step 0 and at every boundary is the restatement at that boundary's weights"""
    cfg = config(tmp_path, "s", sv)
    smc.run_loop(lib, cfg)
    lines = log_of(cfg, "validation_streaming")
    assert [e["step"] for e in lines] == [0] + BOUNDARIES
    changed = set()
    for line in lines:
        metrics, host = restated(lib, cfg, weights_at(cfg, line["step"]) if line["step"] else None)
        same_metrics(line, metrics, line["step"])
        assert host["usable"].all() and metrics["streaming_positives"] == 32 and metrics["streaming_hours"] > 0
        changed.add((metrics["streaming_recall"], metrics["streaming_cutoff"]))
    assert len(changed) > 1   # the boundaries do not all log the same numbers
    return cfg


def check_unnamed_changes_nothing(lib, tmp_path):
    """the key present, the metrics of the best-weights rule left alone: the run without the key, bit for bit - nothing drawn"""
    cfg_a, cfg_s = config(tmp_path, "a"), config(tmp_path, "s", SV)
    model_a, _ = smc.run_loop(lib, cfg_a)
    state_a, opt_a = [w.tobytes() for w in model_a.get_weights()], model_a.engine.get_opt_state()
    model_s, _ = smc.run_loop(lib, cfg_s)
    opt_s = model_s.engine.get_opt_state()
    assert state_a == [w.tobytes() for w in model_s.get_weights()]
    assert opt_a[0].tobytes() == opt_s[0].tobytes() and opt_a[1].tobytes() == opt_s[1].tobytes() and opt_a[2] == opt_s[2] == smc.STEPS
    assert log_bytes(cfg_a, "validation") == log_bytes(cfg_s, "validation") and log_bytes(cfg_a, "train") == log_bytes(cfg_s, "train")
    for name in ("last_weights.weights.h5", "best_weights.weights.h5", os.path.join("restore", "ckpt.weights")):
        assert file_arrays(os.path.join(cfg_a["train_dir"], name)) == file_arrays(os.path.join(cfg_s["train_dir"], name)), name
    assert not os.path.isdir(os.path.join(cfg_a["summaries_dir"], "validation_streaming"))
    assert [e["step"] for e in log_of(cfg_s, "validation_streaming")] == [0] + BOUNDARIES


def preferred(entries, target):
    """the boundary the best-weights rule of train.train keeps, replayed on (step, minimization, maximization) entries"""
    best_min, best_max, best_step = 10000, 0.0, None
    for step, cur_min, cur_max in entries:
        if tr._is_better(cur_min, cur_max, best_min, best_max, target):
            best_min, best_max, best_step = cur_min, cur_max, step
    return best_step


def check_selection_follows_streaming(lib, tmp_path):
    """with the streaming names the rule keeps the boundary the streaming metrics prefer - here not the one accuracy keeps"""
    cfg = config(tmp_path, "n", SV, **STREAMING_NAMES)
    smc.run_loop(lib, cfg)
    lines = [e for e in log_of(cfg, "validation_streaming") if e["step"]]
    by_streaming = preferred([(e["step"], e[STREAMING_NAMES["minimization_metric"]], e[STREAMING_NAMES["maximization_metric"]]) for e in lines],
                             STREAMING_NAMES["target_minimization"])
    by_accuracy = preferred([(e["step"], 0.0, e["accuracy"]) for e in log_of(cfg, "validation")], 0.9)   # the rule of loop_config
    assert by_streaming in BOUNDARIES and by_accuracy in BOUNDARIES and by_streaming != by_accuracy, (by_streaming, by_accuracy, lines)
    best = file_arrays(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    assert best == file_arrays(weights_at(cfg, by_streaming)) and best != file_arrays(weights_at(cfg, by_accuracy))
    # every_evals 2: boundaries 8 and 12 (the last step always) validate, the rule waits at 4
    cfg2 = config(tmp_path, "n2", dict(SV, every_evals=2), **STREAMING_NAMES)
    smc.run_loop(lib, cfg2)
    lines2 = log_of(cfg2, "validation_streaming")
    assert [e["step"] for e in lines2] == [0, 8, 12] and lines2[1:] == lines[1:]
    assert file_arrays(os.path.join(cfg2["train_dir"], "best_weights.weights.h5")) == best


def check_no_window_meets_the_target(lib, tmp_path):
    """the grid ends at cutoff 1.0, which nothing exceeds: only a target below 0 is met by no window.  Recall 0, the fallback
    FAPH (the smallest at the largest cutoff), and the run goes on"""
    cfg = config(tmp_path, "never", dict(SV, target_faph=-1.0), **dict(STREAMING_NAMES, target_minimization=-1.0))
    model, _ = smc.run_loop(lib, cfg)
    lines = log_of(cfg, "validation_streaming")
    assert [e["step"] for e in lines] == [0] + BOUNDARIES and model.engine.get_opt_state()[2] == smc.STEPS
    for e in lines:
        assert e["streaming_recall"] == 0.0 and e["streaming_false_rejection_rate"] == 1.0 and e["streaming_false_accepts_per_hour"] == 0.0
        assert math.isnan(e["streaming_cutoff"]) and e["streaming_window"] == -1 and e["streaming_hours"] > 0 and e["streaming_positives"] == 32
    same_metrics(lines[-1], restated(lib, cfg, weights_at(cfg, smc.STEPS))[0], smc.STEPS)
    # the fallback on a grid that stops below the scores: the smallest FAPH at the largest cutoff over the usable windows
    rng = np.random.default_rng(2)
    amb, pos = [rng.random(400).astype(np.float32), rng.random(300).astype(np.float32)], [rng.random(60).astype(np.float32)]
    g = streaming.operating_summary_host(amb, pos, (5, 2, 500), [0.0, 0.1], target_faph=1.0)
    m = streaming.streaming_metrics(g)
    assert g["recommended"] == -1 and list(g["usable"]) == [True, True, False] and g["faph"][0, 1] != g["faph"][1, 1]
    assert m["streaming_false_accepts_per_hour"] == min(g["faph"][0, 1], g["faph"][1, 1]) > 1.0 and m["streaming_recall"] == 0.0
    assert m["streaming_hours"] == g["hours"][0] and m["streaming_window"] == -1 and math.isnan(m["streaming_cutoff"])


def check_refusals(lib, tmp_path, monkeypatch):
    from microwakeword_amd import mixednet, model_train_eval
    conf = streaming.streaming_validation_config
    for bad, word in ((dict(SV, every=2), "every"), (dict(windows=[5]), "target_faph"), (dict(SV, every_evals=0), "every_evals"),
                      (dict(SV, windows=[]), "windows"), (dict(SV, windows=[5, 257]), "windows"), (dict(SV, windows=list(range(1, 34))), "windows"),
                      (dict(SV, mode="both"), "mode"), (dict(SV, ignore_slices_after_accept=-1), "ignore_slices_after_accept"),
                      (dict(SV, target_faph=float("nan")), "target_faph"), (dict(SV, target_faph="low"), "number"), (dict(SV, data_set=""), "data_set"),
                      (dict(SV, ambient_set=3), "ambient_set"), ([0.5], "mapping")):
        with pytest.raises(ValueError, match="streaming_validation.*" + word):
            conf(dict(streaming_validation=bad))
    assert conf({}) is None and conf(dict(minimization_metric=None, maximization_metric="accuracy")) is None
    assert conf(dict(streaming_validation=dict(target_faph=2))) == dict(
        target_faph=2.0, windows=[5], mode="stream", ignore_slices_after_accept=25, data_set="validation", ambient_set="validation_ambient", every_evals=1)
    assert conf(dict(streaming_validation=dict(SV, windows=7)))["windows"] == [7]
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        conf(dict(streaming_validation=SV), 2)
    # a streaming metric named without the key: before the first step
    model = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    for names in (dict(maximization_metric="streaming_recall"), dict(minimization_metric="streaming_false_accepts_per_hour")):
        cfg = config(tmp_path, "unnamed", **names)
        with pytest.raises(ValueError, match="streaming_validation.*" + list(names.values())[0]):
            tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
        assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    # a handler and a model on two engines
    cfg = config(tmp_path, "two_engines", SV)
    other = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    with pytest.raises(ValueError, match="streaming_validation.*one engine"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=other.engine), verbose=False)
    assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    # a flag set the mode does not cover: spatial attention in stream mode (check_evaluation_topology's refusal)
    attentive = mixednet.model(dict(ec.DEF, spatial_attention=1), (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    cfg = config(tmp_path, "attention", SV)
    with pytest.raises(NotImplementedError, match="spatial_attention"):
        tr.train(attentive, cfg, FeatureHandler(cfg, engine=attentive.engine), verbose=False)
    assert attentive.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    # no usable window: the dry validation, before the first step
    cfg = config(tmp_path, "unusable", dict(SV, windows=[200], ignore_slices_after_accept=90))
    with pytest.raises(ValueError, match="streaming_validation.*usable"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
    assert model.engine.get_opt_state()[2] == 0
    # a world of 2: before the first step
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    cfg = config(tmp_path, "world", SV)
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
    assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    monkeypatch.undo()
    # the command line: before train_dir is claimed (and before a model is built)
    import yaml
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=smc.B_LOOP, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet"]
    for extra, flags, error, word in ((dict(streaming_validation=dict(SV, evry=1)), [], ValueError, "streaming_validation.*evry"),
                                      (dict(streaming_validation=dict(windows=[5])), [], ValueError, "streaming_validation.*target_faph"),
                                      (dict(maximization_metric="streaming_recall"), [], ValueError, "streaming_validation.*streaming_recall"),
                                      (dict(streaming_validation=dict(SV)), ["--spatial_attention", "1", "--residual_connection", "0,0,0,0"], NotImplementedError, "spatial_attention")):
        with open(tmp_path / "training_parameters.yaml", "w") as out:
            yaml.safe_dump(dict(base, **extra), out)
        with pytest.raises(error, match=word):
            model_train_eval.main(argv + flags)
        assert not train_dir.exists()
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    with open(tmp_path / "training_parameters.yaml", "w") as out:
        yaml.safe_dump(dict(base, streaming_validation=dict(SV)), out)
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        model_train_eval.main(argv)
    assert not train_dir.exists()


def check_with_mining(lib, tmp_path):
    """both options in one run: mining at sampling weight 0 leaves the weights alone, so the streaming lines are those of the
    run without it; each option logs at its own boundaries"""
    cfg_s = config(tmp_path, "s", SV)
    model_s, _ = smc.run_loop(lib, cfg_s)
    cfg_b = config(tmp_path, "both", SV, dict(smc.MINING, sampling_weight=0.0))
    model_b, fh_b = smc.run_loop(lib, cfg_b)
    assert [int(e["step"]) for e in smc.mining_log(cfg_b)] == [4, 8] and fh_b.feature_providers[-1].get_mode_size("training") > 0
    assert log_bytes(cfg_b, "validation_streaming") == log_bytes(cfg_s, "validation_streaming")
    assert [a.tobytes() for a in model_s.get_weights()] == [b.tobytes() for b in model_b.get_weights()]
    # and with the mined clips drawn the run differs, and still validates at every boundary
    cfg_d = config(tmp_path, "drawn", SV, smc.MINING)
    model_d, _ = smc.run_loop(lib, cfg_d)
    assert [e["step"] for e in log_of(cfg_d, "validation_streaming")] == [0] + BOUNDARIES
    assert any(a.tobytes() != b.tobytes() for a, b in zip(model_s.get_weights(), model_d.get_weights()))
    same_metrics(log_of(cfg_d, "validation_streaming")[-1], restated(lib, cfg_d, weights_at(cfg_d, smc.STEPS))[0], smc.STEPS)


def check_draws_nothing(lib):
    """one validation leaves Python's and numpy's generators where they stand"""
    cfg = dict(ec.learnable_config(T=smc.T_LOOP), spectrogram_length=smc.T_LOOP)
    from microwakeword_amd import mixednet
    model = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    fh = FeatureHandler(cfg, engine=model.engine)
    state = streaming.StreamingValidation(streaming.streaming_validation_config(dict(streaming_validation=SV)), model, fh, cfg)
    before = mc.rng_state()
    first = state.validate(0)
    assert mc.same_rng(mc.rng_state(), before) and state.validate(0) == first and set(first) == set(streaming.STREAMING_METRICS)
