"""--test_tflite_streaming_quantized with --quantized_backend native on a tiny trained Inception directory, run on the
host-side emulator of the HIP library (MWW_HIP_LIB): calibration, quantization, the reference's folder and ROC file, and the
ROC against the host restatement on the NumPy oracle's probabilities."""
import os

import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_checks as ic
import quant_graph_oracle as qgo
from microwakeword_amd import inception, model_train_eval, native, quantize_graph, streaming
from microwakeword_amd.data import FeatureHandler


def _config(tmp_path, T):
    """ic.cli_config plus the training samples the calibration draws from"""
    cfg = ic.cli_config(tmp_path, T)
    rng = np.random.default_rng(1)
    for feature in cfg["features"]:
        feature["stores"]["training"] = [[rng.integers(0, 900, size=(T, 40)).astype(np.uint16) for _ in range(6)]]
        feature["truncation_strategy"] = "truncate_start"
    return cfg


def test_native_quantized_streaming_of_an_inception_model_writes_the_reference_files(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    T = 60
    cfg = _config(tmp_path, T)
    os.makedirs(cfg["train_dir"])
    flags = model_train_eval.build_parser().parse_args(
        ["--train", "0", "--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "inception"])
    om = ec.perturbed_inception_oracle(T, ec.INC)
    m = inception.model(flags, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    native.NativeLib._instances.pop(emu_lib.path, None)
    out = model_train_eval.evaluate_model(flags, inception, cfg)
    folder = tmp_path / "run" / "tflite_stream_state_internal_quant"
    text = (folder / "tflite_streaming_roc.txt").read_text()
    lines = text.splitlines()
    assert lines[0].startswith("AUC ") and all(l.startswith("Cutoff ") for l in lines[1:])
    assert np.isfinite(out["tflite_stream_state_internal_quant"])
    qm = streaming.load_quantized(str(folder / "stream_state_internal_quant.npz"))
    assert isinstance(qm, quantize_graph.QuantizedGraphModel)
    assert qm.zero_points[0] == -128 and qm.ranges[0, 0] == 0.0 and qm.ranges[0, 1] >= 26.0
    # the ROC on the oracle's probabilities: ambient tracks, then the positives, one stream from zero-point rings
    fh = FeatureHandler(cfg)
    amb, _, _ = fh.get_data("testing_ambient", 0, features_length=T, truncation_strategy="none")
    tst, labels, _ = fh.get_data("testing", 0, features_length=T, truncation_strategy="none")
    pos = [x for x, l in zip(tst, labels) if l == 1.0]
    tracks = list(amb) + pos
    u8, _, _ = qgo.whole_sequence(qm, np.concatenate([np.asarray(x, np.float32) for x in tracks], 0))
    probs = u8.astype(np.float32) * qgo.INV255
    assert len(np.unique(u8)) > 4
    per, at = [], 0
    for x in tracks:
        per.append(probs[at:at + len(x)])
        at += len(x)
    res = streaming.evaluate_probabilities(per[:len(amb)], per[len(amb):], stride=1, step_s=0.02)
    assert res["text"] == text


def test_the_other_quantized_evaluations_of_an_inception_model_still_raise():
    with pytest.raises(NotImplementedError, match="stride-row chunks"):
        model_train_eval.main(["--train", "0", "--test_tflite_nonstreaming_quantized", "1", "--quantized_backend", "native", "inception"])
    with pytest.raises(NotImplementedError, match="--quantized_backend native"):
        model_train_eval.main(["--train", "0", "--test_tflite_streaming_quantized", "1", "inception"])
