"""--operating_point_bootstrap of model_train_eval on a tiny trained directory, run on the host-side emulator of the HIP library
(MWW_HIP_LIB): operating_point_bootstrap.json / operating_point_bootstrap.npz against the NumPy restatement, the files of
--operating_point_faph byte-identical to a run without the flag, misuse refused from the flags alone."""
import json
import os
import random

import numpy as np
import pytest

from microwakeword_amd import model_train_eval, native, streaming
from microwakeword_amd.data import FeatureHandler
from test_operating_points_cli import TARGET, WINDOWS, _run

BOOT = ["--operating_point_bootstrap", "40", "--operating_point_bootstrap_seed", "5", "--operating_point_bootstrap_confidence", "0.8"]
GRID = ["--operating_point_faph", str(TARGET), "--operating_point_windows", ",".join(str(w) for w in WINDOWS)]


def _restated(cfg, model, mode):
    """what the evaluation fed the stream - the ambient tracks, then the positives, the state carried over -, scored again and
    bootstrapped by the NumPy restatement"""
    random.seed(3)
    dp = FeatureHandler(cfg, engine=model.engine)
    sm = streaming.StreamingModel(model, 1, mode)
    off, _ = sm.predict_tracks(dp, "testing_ambient")
    p = sm.read_probabilities()
    amb = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    off, _ = sm.predict_tracks(dp, "testing", only_label=1.0)
    p = sm.read_probabilities()
    pos = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    return streaming.operating_bootstrap_host(amb, pos, WINDOWS, streaming.CUTOFFS, int(cfg["stride"]), cfg["window_step_ms"] / 1000, 25, TARGET,
                                              40, 5, 0, 0.8)


def test_cli_writes_the_bootstrap_and_leaves_the_other_files_alone(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    default = model_train_eval.build_parser().parse_args(["mixednet"])
    assert default.operating_point_bootstrap is None and model_train_eval.operating_point_bootstrap_settings(default) is None   # off by default
    assert (default.operating_point_bootstrap_seed, default.operating_point_bootstrap_block, default.operating_point_bootstrap_confidence) == (0, 0, 0.95)
    _, _, plain = _run(emu_lib, tmp_path, "plain", GRID)
    cfg, model, run = _run(emu_lib, tmp_path, "boot", GRID + BOOT)
    for folder, mode in (("tflite_non_stream", "non_stream"), ("tflite_stream_state_internal", "stream")):
        before = sorted(os.listdir(plain / folder))
        assert before == ["operating_point.json", "operating_points.npz", "operating_points.txt", "tflite_streaming_roc.txt"]
        assert sorted(os.listdir(run / folder)) == sorted(before + ["operating_point_bootstrap.json", "operating_point_bootstrap.npz"])
        for name in before:
            if name.endswith(".npz"):   # a zip archive carries times: compare the arrays
                a, b = np.load(plain / folder / name), np.load(run / folder / name)
                assert a.files == b.files and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files)
            else:
                assert (run / folder / name).read_bytes() == (plain / folder / name).read_bytes(), name
        want = _restated(cfg, model, mode)
        wb = want["bootstrap"]
        r, c = want["recommended"], int(want["chosen"][want["recommended"]])
        assert r >= 0 and (wb["fixed_row"], wb["fixed_cutoff"]) == (r, c)
        z = np.load(run / folder / "operating_point_bootstrap.npz")
        assert sorted(z.files) == sorted(["windows", "cutoffs", "fixed"] + list(native.BOOT_RECORD_DTYPE.names))
        for name in native.BOOT_RECORD_DTYPE.names:
            assert z[name].dtype == wb["records"][name].dtype and z[name].tobytes() == wb["records"][name].tobytes(), name
        assert list(z["fixed"]) == [r, c] and list(z["windows"]) == list(WINDOWS) and z["cutoffs"].tobytes() == streaming.CUTOFFS.tobytes()
        got = json.loads((run / folder / "operating_point_bootstrap.json").read_text())
        settings = json.loads((run / folder / "operating_point.json").read_text())
        assert got == {"replicates": 40, "seed": 5, "block": 0, "confidence": 0.8, "target_false_accepts_per_hour": TARGET,
                       "probability_cutoff": settings["probability_cutoff"], "sliding_window_size": settings["sliding_window_size"],
                       "intervals": {k: list(v) for k, v in wb["intervals"].items()},
                       "replicates_without_operating_point": int(np.count_nonzero(wb["records"]["sel_row"] < 0)), "mode": mode, "quantized": False}
        lo, hi = got["intervals"]["recall"]
        assert lo <= 1 - settings["false_rejection_rate"] <= hi
        lo, hi = got["intervals"]["false_accepts_per_hour"]
        assert lo <= settings["false_accepts_per_hour"] <= hi and wb["records"]["fixed_slices"].min() < wb["records"]["fixed_slices"].max()


@pytest.mark.parametrize("extra, message", [
    (["--operating_point_bootstrap", "100", "--test_tflite_streaming", "1"], "needs --operating_point_faph"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap_seed", "3", "--test_tflite_streaming", "1"], "need --operating_point_bootstrap"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap_block", "1024", "--test_tflite_streaming", "1"], "need --operating_point_bootstrap"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "0", "--test_tflite_streaming", "1"], "operating_point_bootstrap.*replicates"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "65537", "--test_tflite_streaming", "1"], "operating_point_bootstrap.*replicates"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "10", "--operating_point_bootstrap_block", "1000", "--test_tflite_streaming", "1"],
     "operating_point_bootstrap.*block"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "10", "--operating_point_bootstrap_confidence", "1", "--test_tflite_streaming", "1"],
     "operating_point_bootstrap.*confidence"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "10", "--operating_point_bootstrap_seed", "-1", "--test_tflite_streaming", "1"],
     "operating_point_bootstrap.*seed"),
    (["--operating_point_faph", "1", "--operating_point_bootstrap", "10"], "needs --test_tflite_nonstreaming"),
])
def test_cli_refuses_misuse_from_the_flags_alone(tmp_path, monkeypatch, extra, message):
    # the configuration file does not exist: the refusal comes before it is read, before training, before train_dir is claimed
    monkeypatch.chdir(tmp_path)
    for train in ("0", "1"):
        with pytest.raises(ValueError, match=message):
            model_train_eval.main(["--training_config", str(tmp_path / "none.yaml"), "--train", train] + extra + ["mixednet"])
    assert os.listdir(tmp_path) == []
