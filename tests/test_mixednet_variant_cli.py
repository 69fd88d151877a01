"""The evaluation flags of model_train_eval on a saved residual + pooled MixedNet (--train 0 with --test_tf_nonstreaming,
--test_tflite_nonstreaming and --test_tflite_streaming), run on the host-side emulator of the HIP library (MWW_HIP_LIB): the
three result files against ``streaming.evaluate_probabilities`` on the float64 oracle's probabilities."""
import os

import numpy as np

import engine_checks as ec
import mixednet_variant_streaming_oracle as vo
import streaming_oracle as so
from microwakeword_amd import mixednet, model_train_eval, native, streaming



def _config(tmp_path, T):
    """a tiny test set in the layout FeatureHandler reads: positives, negatives and two ambient tracks, uint16 features"""
    rng = np.random.default_rng(0)

    def samples(n, lo, hi):
        return [[rng.integers(0, 900, size=(int(rng.integers(lo, hi)), 40)).astype(np.uint16) for _ in range(n)]]
    pos = {"testing": samples(6, T + 40, T + 80)}   # long enough for 30 non-streaming windows
    neg = {"testing": samples(4, T, T + 30), "testing_ambient": samples(2, 3 * T, 4 * T)}
    return {"stride": 1, "window_step_ms": 20, "train_dir": str(tmp_path / "run"), "batch_size": 8, "spectrogram_length": T,
            "training_input_shape": (T, 40),
            "features": [dict(type="mmap", stores=pos, truth=True, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
                         dict(type="mmap", stores=neg, truth=False, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="split")]}


FLAGS = dict(ec.GRAPH_MIXEDNET, residual_connection="1,0,1", pooled=1, stride=1)
T = 40


def test_cli_evaluates_a_residual_pooled_model(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    cfg = _config(tmp_path, T)
    os.makedirs(cfg["train_dir"])
    om = ec.perturbed_oracle(T, flags=FLAGS)
    m = mixednet.model(FLAGS, (T, 40), 8, lib=emu_lib, max_batch=16)
    m.set_weights(om.get_weights())
    m.save_weights(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    argv = ["--train", "0", "--test_tf_nonstreaming", "1", "--test_tflite_nonstreaming", "1", "--test_tflite_streaming", "1", "mixednet"]
    for k in ("residual_connection", "pointwise_filters", "repeat_in_block", "mixconv_kernel_sizes", "first_conv_filters",
              "first_conv_kernel_size", "stride", "pooled"):
        argv += ["--" + k, str(FLAGS[k])]
    flags = model_train_eval.build_parser().parse_args(argv)
    model_train_eval.check_evaluation_flags(flags, mixednet, cfg)   # what _run asks before anything else
    native.NativeLib._instances.pop(emu_lib.path, None)
    out = model_train_eval.evaluate_model(flags, mixednet, cfg)
    run = tmp_path / "run"
    text = (run / "non_stream" / "testing_set_metrics.txt").read_text()
    # --test_tf_nonstreaming: the oracle on the last T frames of every test sample (truncate_start), p > 0.5 against the label
    neg_t = [np.asarray(a, np.float64) * 0.0390625 for a in cfg["features"][1]["stores"]["testing"][0]]
    pos_t = [np.asarray(a, np.float64) * 0.0390625 for a in cfg["features"][0]["stores"]["testing"][0]]
    p_pos = om.predict_with_logits(np.stack([t[len(t) - T:] for t in pos_t]))[0]
    p_neg = om.predict_with_logits(np.stack([t[len(t) - T:] for t in neg_t]))[0]
    assert np.abs(np.concatenate([p_pos, p_neg]) - 0.5).min() > 1e-4   # no decision within the float32 error of the threshold
    tp, fp = int((p_pos > 0.5).sum()), int((p_neg > 0.5).sum())
    want = streaming.compute_metrics(tp, len(p_neg) - fp, fp, len(p_pos) - tp)
    assert text == streaming.metrics_to_string(want), (text, streaming.metrics_to_string(want))
    assert out["non_stream"]["count"] == 10

    # the oracle's probabilities on the same tracks: the ambient tracks, then the positive tracks of the test set, through one
    # stream from zero state (stream mode), or window by window (non_stream mode)
    pos = [np.asarray(a, np.float64) * 0.0390625 for a in cfg["features"][0]["stores"]["testing"][0]]
    amb = [np.asarray(a, np.float64) * 0.0390625 for a in cfg["features"][1]["stores"]["testing_ambient"][0]]
    net = vo.Net(FLAGS, om, T)
    z = vo.whole_sequence(net, np.concatenate(amb + pos, 0))
    cuts = np.cumsum([0] + [len(t) for t in amb + pos])
    stream_p = [so.sigmoid(z[a:b]).astype(np.float32) for a, b in zip(cuts, cuts[1:])]
    ns_p = [so.sigmoid(so.non_stream_windows(om, t, T, 1)).astype(np.float32) for t in amb + pos]
    for folder, probs in (("tflite_stream_state_internal", stream_p), ("tflite_non_stream", ns_p)):
        want = streaming.evaluate_probabilities(probs[:len(amb)], probs[len(amb):], stride=1, step_s=0.02)
        got = (run / folder / "tflite_streaming_roc.txt").read_text()
        assert got.splitlines()[0] == "AUC {:.5f}".format(want["auc"]) and abs(out[folder] - want["auc"]) < 5e-6
        assert got == want["text"], (folder, got, want["text"])
