"""--detections_cutoff of model_train_eval on a tiny trained directory, run on the host-side emulator of the HIP library
(MWW_HIP_LIB): detections.txt / detections.npz against the NumPy restatement, the ROC files byte-identical to a run without
the flag."""
import os
import random

import numpy as np

import engine_checks as ec
from microwakeword_amd import mixednet, model_train_eval, native, streaming
from microwakeword_amd.data import FeatureHandler
from test_streaming_cli import _config

CUTOFF = 0.5425   # inside the narrow band of this tiny perturbed model's probabilities: some fire, some positives are missed


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


def _restated(cfg, model, mode, cutoff, w=5, ignore=25):
    """what the evaluation fed the stream, scored again and located by the NumPy restatement"""
    random.seed(3)
    dp = FeatureHandler(cfg, engine=model.engine)
    sm = streaming.StreamingModel(model, 1, mode)
    off, _ = sm.predict_tracks(dp, "testing_ambient")
    p = sm.read_probabilities()
    mas = [streaming.moving_average_in_order(p[off[t]:off[t + 1]], w) for t in range(off.size - 1)]
    at = streaming.detection_positions(mas, cutoff, ignore)
    amb = [(t, int(i), mas[t][i]) for t in range(len(mas)) for i in at[t]]
    off, _ = sm.predict_tracks(dp, "testing", only_label=1.0)   # the state carries over from the ambient tracks
    p = sm.read_probabilities()
    pos = [streaming.moving_average_in_order(p[off[t]:off[t + 1]][ignore:], w) for t in range(off.size - 1)]
    return amb, [(t, np.max(ma), int(np.argmax(ma))) for t, ma in enumerate(pos)]


def test_cli_writes_detections_and_leaves_the_roc_alone(emu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("MWW_HIP_LIB", emu_lib.path)
    assert model_train_eval.build_parser().parse_args(["mixednet"]).detections_cutoff is None   # off by default
    _, _, plain = _run(emu_lib, tmp_path, "plain", [])
    cfg, model, run = _run(emu_lib, tmp_path, "located", ["--detections_cutoff", str(CUTOFF)])
    located, n_missed = 0, 0
    for folder, mode in (("tflite_non_stream", "non_stream"), ("tflite_stream_state_internal", "stream")):
        assert (run / folder / "tflite_streaming_roc.txt").read_bytes() == (plain / folder / "tflite_streaming_roc.txt").read_bytes()
        assert sorted(os.listdir(plain / folder)) == ["tflite_streaming_roc.txt"]
        assert sorted(os.listdir(run / folder)) == ["detections.npz", "detections.txt", "tflite_streaming_roc.txt"]
        amb, pos = _restated(cfg, model, mode, CUTOFF)
        missed = [(t, s, i) for t, s, i in pos if not s > CUTOFF]
        want = ["Cutoff {:.4f}: {} ambient false accepts, {} of {} positives missed".format(CUTOFF, len(amb), len(missed), len(pos))]
        want += ["ambient track {}: t={:.3f} s; average={:.6f}".format(t, i * 1 * 20 / 1000, float(a)) for t, i, a in amb]
        want += ["missed positive track {}: score={:.6f}; t={:.3f} s".format(t, float(s), i * 1 * 20 / 1000) for t, s, i in missed]
        assert (run / folder / "detections.txt").read_text().splitlines() == want
        z = np.load(run / folder / "detections.npz")
        assert list(z["ambient_track"]) == [t for t, _, _ in amb] and list(z["ambient_index"]) == [i for _, i, _ in amb]
        assert z["ambient_average"].tobytes() == np.array([a for _, _, a in amb], np.float32).tobytes()
        assert np.array_equal(z["ambient_seconds"], z["ambient_index"] * 0.02)
        assert z["positive_score"].tobytes() == np.array([s for _, s, _ in pos], np.float32).tobytes()
        assert list(z["positive_best_index"]) == [i for _, _, i in pos] and list(z["missed_positive_track"]) == [t for t, _, _ in missed]
        located += len(amb)
        n_missed += len(missed)
    assert located > 0 and n_missed > 0
