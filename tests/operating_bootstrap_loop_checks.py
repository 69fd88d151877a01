"""Checks of the ``bootstrap`` sub-mapping of ``streaming_validation`` (streaming.validate_streaming, train.train), shared by the
emulator tests (tests/test_operating_bootstrap_loop_emulated.py) and the GPU test (tests/test_operating_bootstrap_loop_gpu.py).
The loop is the tiny run of tests/stream_mine_checks.py (12 steps, boundaries at 4, 8 and 12); every comparison is exact: the
logged bounds against ``streaming.operating_bootstrap_host`` on the probabilities read back at the same weights, logs and weights
byte for byte."""
import json
import logging
import os
import random

import numpy as np
import pytest

from microwakeword_amd import native, streaming
from microwakeword_amd import train as tr
from microwakeword_amd.data import FeatureHandler
import engine_checks as ec
import mining_checks as mc
import stream_mine_checks as smc
import streaming_validation_checks as svc

BOOT = dict(replicates=60, seed=3, confidence=0.9, block=0)
SVB = dict(svc.SV, bootstrap=BOOT)
NAMES = dict(minimization_metric="streaming_false_accepts_per_hour", maximization_metric="streaming_recall_lower", target_minimization=0.5)
ALL_NAMES = streaming.STREAMING_METRICS + streaming.STREAMING_BOOTSTRAP_METRICS


def restated(lib, cfg, weights=None):
    """svc.restated with the bootstrap: the metrics of a fresh model at the run's initial weights or at a weights file of the
    run, by the host restatement on the probabilities read back"""
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
    b = v["bootstrap"]
    host = streaming.operating_bootstrap_host(tracks[:amb.size], tracks[amb.size:], v["windows"], streaming.CUTOFFS, sm.stride,
                                              cfg["window_step_ms"] / 1000, v["ignore_slices_after_accept"], v["target_faph"], b["replicates"],
                                              b["seed"], b["block"], b["confidence"])
    return streaming.streaming_metrics(host), host


def check_loop(lib, tmp_path, rerun=True):
    """the six bounds are logged at step 0 and at every boundary, equal the restatement at that boundary's weights, the rule
    keeps the boundary ``streaming_recall_lower`` prefers, and the same configuration writes the same files again"""
    cfg = svc.config(tmp_path, "b", SVB, **NAMES)
    smc.run_loop(lib, cfg)
    lines = svc.log_of(cfg, "validation_streaming")
    assert [e["step"] for e in lines] == [0] + svc.BOUNDARIES
    seen = set()
    for line in lines:
        assert list(line) == ["step"] + list(ALL_NAMES), list(line)
        metrics, host = restated(lib, cfg, svc.weights_at(cfg, line["step"]) if line["step"] else None)
        assert list(metrics) == list(ALL_NAMES) and all(line[k] == float(v) for k, v in metrics.items()), (line, metrics)
        for name in ("streaming_recall", "streaming_false_accepts_per_hour", "streaming_recall_at_target"):
            assert line[name + "_lower"] <= line[name + "_upper"], (name, line)
        # the point estimate at the fixed point lies inside what its own replicates span
        rec = host["bootstrap"]["records"]
        assert rec.shape == (BOOT["replicates"],) and host["bootstrap"]["fixed_row"] == host["recommended"] >= 0
        assert rec["fixed_accepts"].min() <= host["accepts"][host["recommended"], host["chosen"][host["recommended"]]] <= rec["fixed_accepts"].max()
        seen.add((line["streaming_recall_lower"], line["streaming_recall_upper"]))
    assert len(seen) > 1   # the boundaries do not all log the same bounds (the synthetic set separates: the intervals are narrow)
    entries = [(e["step"], e[NAMES["minimization_metric"]], e[NAMES["maximization_metric"]]) for e in lines if e["step"]]
    kept = svc.preferred(entries, NAMES["target_minimization"])
    assert kept in svc.BOUNDARIES
    best = svc.file_arrays(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    assert best == svc.file_arrays(svc.weights_at(cfg, kept))
    if rerun:
        cfg2 = svc.config(tmp_path, "b2", SVB, **NAMES)
        smc.run_loop(lib, cfg2)
        for which in ("validation_streaming", "validation", "train"):
            assert svc.log_bytes(cfg, which) == svc.log_bytes(cfg2, which), which
        assert svc.file_arrays(os.path.join(cfg2["train_dir"], "best_weights.weights.h5")) == best
    return cfg, lines


def check_without_the_sub_mapping(lib, tmp_path, caplog):
    """the sub-mapping adds six scalars and one log line and changes nothing else: the run without it writes the lines of the
    run with it less the six keys, byte for byte, the same training and validation logs and weights, and logs no bootstrap line"""
    caplog.set_level(logging.INFO, logger="microwakeword_amd.train")
    cfg_s = svc.config(tmp_path, "s", svc.SV)
    model_s, _ = smc.run_loop(lib, cfg_s)
    plain_log = [r.getMessage() for r in caplog.records if r.name == "microwakeword_amd.train"]
    caplog.clear()
    cfg_b = svc.config(tmp_path, "b", SVB)
    model_b, _ = smc.run_loop(lib, cfg_b)
    boot_log = [r.getMessage() for r in caplog.records if r.name == "microwakeword_amd.train"]
    assert [a.tobytes() for a in model_s.get_weights()] == [b.tobytes() for b in model_b.get_weights()]
    for which in ("validation", "train"):
        assert svc.log_bytes(cfg_s, which) == svc.log_bytes(cfg_b, which), which
    stripped = b"".join((json.dumps({k: v for k, v in e.items() if k not in streaming.STREAMING_BOOTSTRAP_METRICS}) + "\n").encode()
                        for e in svc.log_of(cfg_b, "validation_streaming"))
    assert svc.log_bytes(cfg_s, "validation_streaming") == stripped
    assert all(set(e) == set(streaming.STREAMING_METRICS) | {"step"} for e in svc.log_of(cfg_s, "validation_streaming"))
    extra = [m for m in boot_log if "bootstrap" in m]
    assert len(extra) == 1 + len(svc.BOUNDARIES) and all("percentile intervals of 60 replicates" in m for m in extra)
    assert not any("bootstrap" in m for m in plain_log) and [m for m in boot_log if "bootstrap" not in m] == plain_log


def check_draws_nothing(lib):
    """one validation with the bootstrap leaves Python's and numpy's generators where they stand, and repeats itself"""
    cfg = dict(ec.learnable_config(T=smc.T_LOOP), spectrogram_length=smc.T_LOOP)
    from microwakeword_amd import mixednet
    model = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    fh = FeatureHandler(cfg, engine=model.engine)
    state = streaming.StreamingValidation(streaming.streaming_validation_config(dict(streaming_validation=SVB)), model, fh, cfg)
    before = mc.rng_state()
    first = state.validate(0)
    assert mc.same_rng(mc.rng_state(), before) and state.validate(0) == first and list(first) == list(ALL_NAMES)
    assert state.last["bootstrap"]["records"].dtype == native.BOOT_RECORD_DTYPE
    plain = streaming.StreamingValidation(streaming.streaming_validation_config(dict(streaming_validation=svc.SV)), model, fh, cfg).validate(0)
    assert plain == {k: first[k] for k in streaming.STREAMING_METRICS}


def check_refusals(lib, tmp_path, monkeypatch):
    conf = streaming.streaming_validation_config
    for bad, word in ((dict(replicates=0), "replicates"), (dict(replicates=native.BOOT_MAX_REPLICATES + 1), "replicates"), (dict(replicates=2.5), "replicates"),
                      (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(confidence=1.0), "confidence"), (dict(confidence=0), "confidence"),
                      (dict(confidence="high"), "confidence"), (dict(block=1000), "block"), (dict(block=-1024), "block"), (dict(block=True), "block"),
                      (dict(reps=5), "reps"), ([100], "mapping"), (100, "mapping")):
        with pytest.raises(ValueError, match="streaming_validation: bootstrap.*" + word):
            conf(dict(streaming_validation=dict(svc.SV, bootstrap=bad)))
    assert "bootstrap" not in conf(dict(streaming_validation=svc.SV))
    assert conf(dict(streaming_validation=dict(svc.SV, bootstrap={})))["bootstrap"] == dict(replicates=1000, seed=0, confidence=0.95, block=0)
    assert conf(dict(streaming_validation=dict(svc.SV, bootstrap=dict(block=2048, seed=2 ** 64 - 1))))["bootstrap"] == dict(
        replicates=1000, seed=2 ** 64 - 1, confidence=0.95, block=2048)
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        conf(dict(streaming_validation=SVB), 2)
    # a bound named without the sub-mapping, or without the mapping: before the first step
    from microwakeword_amd import mixednet, model_train_eval
    model = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    for sv, word in ((svc.SV, "streaming_recall_lower needs the bootstrap sub-mapping"), (None, "streaming_recall_lower needs the streaming_validation mapping")):
        cfg = svc.config(tmp_path, "unnamed", sv, maximization_metric="streaming_recall_lower")
        with pytest.raises(ValueError, match="streaming_validation.*" + word):
            tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
        assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    cfg = svc.config(tmp_path, "bad", dict(svc.SV, bootstrap=dict(block=1000)))
    with pytest.raises(ValueError, match="streaming_validation: bootstrap.*block"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
    assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    cfg = svc.config(tmp_path, "world", SVB)
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
    assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    monkeypatch.undo()
    # the command line: before train_dir is claimed (and before a model is built)
    import yaml
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=smc.B_LOOP, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet"]
    for extra, word in ((dict(streaming_validation=dict(svc.SV, bootstrap=dict(replicates=0))), "bootstrap.*replicates"),
                        (dict(streaming_validation=dict(svc.SV, bootstrap=dict(blok=0))), "bootstrap.*blok"),
                        (dict(streaming_validation=dict(svc.SV), maximization_metric="streaming_recall_at_target_lower"), "bootstrap sub-mapping")):
        with open(tmp_path / "training_parameters.yaml", "w") as out:
            yaml.safe_dump(dict(base, **extra), out)
        with pytest.raises(ValueError, match="streaming_validation.*" + word):
            model_train_eval.main(argv)
        assert not train_dir.exists()
