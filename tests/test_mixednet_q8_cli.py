"""--test_tflite_streaming_quantized with --quantized_backend native_ext on a tiny trained directory of a residual + pooled
MixedNet, run on the host-side emulator of the HIP library (MWW_HIP_LIB): calibration, quantization, the reference's folder,
the ``.npz`` and the ROC file against the host restatement on the NumPy oracle's probabilities."""
import os

import numpy as np
import pytest

import engine_checks as ec
import quant_mixednet_oracle as qmo
from microwakeword_amd import mixednet, model_train_eval, native, quantize_mixednet, streaming
from microwakeword_amd.data import FeatureHandler

FLAGS = dict(ec.GRAPH_MIXEDNET, residual_connection="1,0,1", pooled=1, stride=1)
T = 40


def _config(tmp_path):
    rng = np.random.default_rng(0)

    def samples(n, lo, hi):
        return [[rng.integers(0, 900, size=(int(rng.integers(lo, hi)), 40)).astype(np.uint16) for _ in range(n)]]
    pos = {"training": samples(6, T, T + 1), "testing": samples(6, T + 40, T + 80)}
    neg = {"training": samples(6, T, T + 1), "testing": samples(4, T, T + 30), "testing_ambient": samples(2, 3 * T, 4 * T)}
    return {"stride": 1, "window_step_ms": 20, "train_dir": str(tmp_path / "run"), "batch_size": 8, "spectrogram_length": T,
            "training_input_shape": (T, 40),
            "features": [dict(type="mmap", stores=pos, truth=True, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
                         dict(type="mmap", stores=neg, truth=False, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="truncate_start")]}


def _argv(backend):
    argv = ["--train", "0", "--test_tflite_streaming_quantized", "1", "--quantized_backend", backend, "mixednet"]
    for k in ("residual_connection", "pointwise_filters", "repeat_in_block", "mixconv_kernel_sizes", "first_conv_filters",
              "first_conv_kernel_size", "stride", "pooled"):
        argv += ["--" + k, str(FLAGS[k])]
    return argv


def test_native_ext_writes_the_reference_files_of_a_residual_pooled_model(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    cfg = _config(tmp_path)
    os.makedirs(cfg["train_dir"])
    om = ec.perturbed_oracle(T, flags=FLAGS)
    m = mixednet.model(FLAGS, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    flags = model_train_eval.build_parser().parse_args(_argv("native_ext"))
    model_train_eval.check_evaluation_flags(flags, mixednet, cfg)   # what _run asks before anything else
    with pytest.raises(NotImplementedError, match="residual_connection, pooled.*native_ext"):
        model_train_eval.check_evaluation_flags(model_train_eval.build_parser().parse_args(_argv("native")), mixednet, cfg)
    native.NativeLib._instances.pop(emu_lib.path, None)
    out = model_train_eval.evaluate_model(flags, mixednet, cfg)
    folder = tmp_path / "run" / "tflite_stream_state_internal_quant"
    text = (folder / "tflite_streaming_roc.txt").read_text()
    lines = text.splitlines()
    assert lines[0].startswith("AUC ") and all(l.startswith("Cutoff ") for l in lines[1:])
    assert np.isfinite(out["tflite_stream_state_internal_quant"])
    qm = streaming.load_quantized(str(folder / "stream_state_internal_quant.npz"))
    assert isinstance(qm, quantize_mixednet.QuantizedMixedNetModel)
    assert qm.desc["residual"] == [1, 0, 1] and qm.desc["pool"] == "average" and qm.desc["t_final"] > 1
    assert qm.names == quantize_mixednet.tensor_names(qm.desc) and "block0.residual" in qm.names and "block2.r0.add" in qm.names
    assert qm.zero_points[0] == -128 and qm.ranges[0, 0] == 0.0 and qm.ranges[0, 1] >= 26.0
    # the ROC on the oracle's probabilities: ambient tracks, then the positives, one stream from zero-point rings
    fh = FeatureHandler(cfg)
    amb, _, _ = fh.get_data("testing_ambient", 0, features_length=T, truncation_strategy="none")
    tst, labels, _ = fh.get_data("testing", 0, features_length=T, truncation_strategy="none")
    pos = [x for x, l in zip(tst, labels) if l == 1.0]
    tracks = list(amb) + pos
    u8, lq, _ = qmo.whole_sequence(qm, np.concatenate([np.asarray(x, np.float32) for x in tracks], 0))
    assert len(np.unique(lq)) >= 16
    probs = u8.astype(np.float32) * qmo.INV255
    per, at = [], 0
    for x in tracks:
        per.append(probs[at:at + len(x)])
        at += len(x)
    res = streaming.evaluate_probabilities(per[:len(amb)], per[len(amb):], stride=1, step_s=0.02)
    assert res["text"] == text
