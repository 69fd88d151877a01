"""The evaluation flags of model_train_eval (--test_tf_nonstreaming / --test_tflite_nonstreaming / --test_tflite_streaming)
on a tiny trained directory, run on the host-side emulator of the HIP library (MWW_HIP_LIB)."""
import os

import numpy as np
import pytest

import engine_checks as ec
from microwakeword_amd import mixednet, model_train_eval, native


def _config(tmp_path, T):
    rng = np.random.default_rng(0)

    def samples(n, lo, hi):
        return [[rng.integers(0, 900, size=(int(rng.integers(lo, hi)), 40)).astype(np.uint16) for _ in range(n)]]
    pos = {"testing": samples(6, T + 40, T + 80)}   # long enough for 30 non-streaming windows
    neg = {"testing": samples(4, T, T + 30), "testing_ambient": samples(2, 3 * T, 4 * T)}
    return {"stride": 1, "window_step_ms": 20, "train_dir": str(tmp_path / "run"), "batch_size": 8, "spectrogram_length": T,
            "training_input_shape": (T, 40),
            "features": [dict(type="mmap", stores=pos, truth=True, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
                         dict(type="mmap", stores=neg, truth=False, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="split")]}


def test_cli_evaluation_writes_the_three_files(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    T = 52
    cfg = _config(tmp_path, T)
    os.makedirs(cfg["train_dir"])
    om = ec.perturbed_oracle(T, flags=ec.DEF)
    m = mixednet.model(ec.DEF, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    flags = model_train_eval.build_parser().parse_args(
        ["--train", "0", "--test_tf_nonstreaming", "1", "--test_tflite_nonstreaming", "1", "--test_tflite_streaming", "1",
         "mixednet", "--residual_connection", "0,0,0,0"])
    native.NativeLib._instances.pop(emu_lib.path, None)
    out = model_train_eval.evaluate_model(flags, mixednet, cfg)
    run = tmp_path / "run"
    text = (run / "non_stream" / "testing_set_metrics.txt").read_text()
    assert text.startswith("accuracy = ") and "(N=10)" in text
    for folder in ("tflite_non_stream", "tflite_stream_state_internal"):
        lines = (run / folder / "tflite_streaming_roc.txt").read_text().splitlines()
        assert lines[0].startswith("AUC ") and all(l.startswith("Cutoff ") for l in lines[1:])
        assert np.isfinite(out[folder])


def test_quantized_flags_still_raise():
    with pytest.raises(NotImplementedError, match="--test_tflite_streaming run here"):
        model_train_eval.main(["--train", "0", "--test_tflite_streaming_quantized", "1", "mixednet"])
    with pytest.raises(NotImplementedError, match="quantized"):
        model_train_eval.main(["--train", "0", "--test_tflite_nonstreaming_quantized", "1", "mixednet"])
