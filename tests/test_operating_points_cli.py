"""--operating_point_faph of model_train_eval on a tiny trained directory, run on the host-side emulator of the HIP library
(MWW_HIP_LIB): operating_points.txt / operating_points.npz / operating_point.json against the NumPy restatement, the ROC files
byte-identical to a run without the flag, misuse refused from the flags alone."""
import json
import os
import random

import numpy as np
import pytest

import engine_checks as ec
from microwakeword_amd import mixednet, model_train_eval, native, streaming
from microwakeword_amd.data import FeatureHandler
from test_streaming_cli import _config

TARGET = 1000.0   # the ambient tracks last seconds: one count is some 500 false accepts per hour
WINDOWS = (5, 1, 12)


def _run(emu_lib, tmp_path, name, extra):
    T = 52
    cfg = _config(tmp_path / name, T)
    os.makedirs(cfg["train_dir"])
    om = ec.perturbed_oracle(T, flags=ec.DEF)
    m = mixednet.model(ec.DEF, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    flags = model_train_eval.build_parser().parse_args(
        ["--train", "0", "--test_tflite_nonstreaming", "1", "--test_tflite_streaming", "1"] + extra
        + ["mixednet", "--residual_connection", "0,0,0,0"])
    native.NativeLib._instances.pop(emu_lib.path, None)
    random.seed(3)   # the handler shuffles its track lists on the global generator: _restated repeats it
    model_train_eval.evaluate_model(flags, mixednet, cfg)
    return cfg, m, tmp_path / name / "run"


def _restated(cfg, model, mode):
    """what the evaluation fed the stream, scored again and gridded by the NumPy restatement"""
    random.seed(3)
    dp = FeatureHandler(cfg, engine=model.engine)
    sm = streaming.StreamingModel(model, 1, mode)
    off, _ = sm.predict_tracks(dp, "testing_ambient")
    p = sm.read_probabilities()
    amb = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    off, _ = sm.predict_tracks(dp, "testing", only_label=1.0)   # the state carries over from the ambient tracks
    p = sm.read_probabilities()
    pos = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    return streaming.operating_points_host(amb, pos, WINDOWS, target_faph=TARGET)


def test_cli_writes_the_operating_point_and_leaves_the_roc_alone(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    default = model_train_eval.build_parser().parse_args(["mixednet"])
    assert default.operating_point_faph is None and default.operating_point_windows == "1,2,3,4,5,6,7,8,9,10"   # off by default
    assert tuple(int(w) for w in default.operating_point_windows.split(",")) == streaming.OP_WINDOWS
    _, _, plain = _run(emu_lib, tmp_path, "plain", [])
    cfg, model, run = _run(emu_lib, tmp_path, "chosen", ["--operating_point_faph", str(TARGET), "--operating_point_windows",
                                                         ",".join(str(w) for w in WINDOWS)])
    for folder, mode in (("tflite_non_stream", "non_stream"), ("tflite_stream_state_internal", "stream")):
        assert (run / folder / "tflite_streaming_roc.txt").read_bytes() == (plain / folder / "tflite_streaming_roc.txt").read_bytes()
        assert sorted(os.listdir(plain / folder)) == ["tflite_streaming_roc.txt"]
        assert sorted(os.listdir(run / folder)) == ["operating_point.json", "operating_points.npz", "operating_points.txt", "tflite_streaming_roc.txt"]
        want = _restated(cfg, model, mode)
        assert want["usable"].all() and want["recommended"] >= 0 and want["counts"].any()
        z = np.load(run / folder / "operating_points.npz")
        assert sorted(z.files) == ["chosen_cutoff", "counts", "cutoffs", "faph", "frr", "hours", "recommended", "windows"]
        for name in ("windows", "cutoffs", "counts", "faph", "frr", "hours", "chosen_cutoff"):
            assert z[name].dtype == want[name].dtype and z[name].tobytes() == want[name].tobytes(), name
        assert int(z["recommended"]) == want["recommended"]
        assert (run / folder / "operating_points.txt").read_text() == streaming.operating_point_text(want)
        # the settings are the rule's answer on the restated grid
        chosen, rec = streaming.select_operating_points(want["faph"], want["frr"], want["usable"], TARGET, WINDOWS)
        c = chosen[rec]
        settings = json.loads((run / folder / "operating_point.json").read_text())
        assert settings == {"probability_cutoff": float(streaming.CUTOFFS[c]), "sliding_window_size": WINDOWS[rec],
                            "false_accepts_per_hour": float(want["faph"][rec, c]), "false_rejection_rate": float(want["frr"][rec, c]),
                            "target_false_accepts_per_hour": TARGET, "mode": mode, "quantized": False}
        assert want["faph"][rec, c] <= TARGET and (c == 0 or want["faph"][rec, c - 1] > TARGET)


@pytest.mark.parametrize("extra, message", [
    (["--operating_point_faph", "0", "--test_tflite_streaming", "1"], "positive"),
    (["--operating_point_faph", "-2", "--test_tflite_streaming", "1"], "positive"),
    (["--operating_point_faph", "1", "--operating_point_windows", "5,0", "--test_tflite_streaming", "1"], "1..256"),
    (["--operating_point_faph", "1", "--operating_point_windows", "257", "--test_tflite_nonstreaming", "1"], "1..256"),
    (["--operating_point_faph", "1", "--operating_point_windows", ",".join(["5"] * 33), "--test_tflite_streaming", "1"], "1..32 windows"),
    (["--operating_point_faph", "1", "--operating_point_windows", "five", "--test_tflite_streaming", "1"], "integers"),
    (["--operating_point_faph", "1"], "needs --test_tflite_nonstreaming"),
    (["--operating_point_faph", "1", "--test_tf_nonstreaming", "1"], "needs --test_tflite_nonstreaming"),
])
def test_cli_refuses_misuse_from_the_flags_alone(tmp_path, monkeypatch, extra, message):
    # the configuration file does not exist: the refusal comes before it is read, before training, before train_dir is claimed
    monkeypatch.chdir(tmp_path)
    for train in ("0", "1"):
        with pytest.raises(ValueError, match=message):
            model_train_eval.main(["--training_config", str(tmp_path / "none.yaml"), "--train", train] + extra + ["mixednet"])
    assert os.listdir(tmp_path) == []
    assert model_train_eval.operating_point_windows(model_train_eval.build_parser().parse_args(
        ["--operating_point_faph", "0.5", "--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "mixednet"])) == list(range(1, 11))
