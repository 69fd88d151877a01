"""The evaluation flags of model_train_eval (--test_tf_nonstreaming / --test_tflite_nonstreaming / --test_tflite_streaming)
on a tiny trained Inception directory, run on the host-side emulator of the HIP library (MWW_HIP_LIB)."""
import os

import numpy as np

import engine_checks as ec
from microwakeword_amd import inception, model_train_eval, native
import inception_streaming_checks as ic


def test_cli_evaluation_of_an_inception_model_writes_the_three_files(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    T = 60
    cfg = ic.cli_config(tmp_path, T)
    os.makedirs(cfg["train_dir"])
    flags = model_train_eval.build_parser().parse_args(
        ["--train", "0", "--test_tf_nonstreaming", "1", "--test_tflite_nonstreaming", "1", "--test_tflite_streaming", "1", "inception"])
    om = ec.perturbed_inception_oracle(T, ec.INC)
    m = inception.model(flags, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    native.NativeLib._instances.pop(emu_lib.path, None)
    out = model_train_eval.evaluate_model(flags, inception, cfg)
    run = tmp_path / "run"
    text = (run / "non_stream" / "testing_set_metrics.txt").read_text()
    assert text.startswith("accuracy = ") and "(N=10)" in text
    for folder in ("tflite_non_stream", "tflite_stream_state_internal"):
        lines = (run / folder / "tflite_streaming_roc.txt").read_text().splitlines()
        assert lines[0].startswith("AUC ") and all(l.startswith("Cutoff ") for l in lines[1:])
        assert np.isfinite(out[folder]) and np.isfinite(float(lines[0].split()[1]))
