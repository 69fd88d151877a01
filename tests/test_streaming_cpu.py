"""Streaming evaluation, host side: the two float64 restatements of the streaming MixedNet agree with each other and with the
non-streaming graph after warm-up; the restated FAPH / FRR / ROC post-processing reproduces what the reference's own test.py
computes (tests/golden/streaming_metrics_golden.npz); ``get_data(..., "none")``."""
import os
import random
import sys

import numpy as np
import pytest

import engine_checks as ec
import streaming_oracle as so
from microwakeword_amd import streaming

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_metrics_golden.npz")
TOPOLOGIES = {"DEF": (ec.DEF, 52), "NOTEBOOK": (ec.NOTEBOOK, 164), "GRAPH_MIXEDNET": (ec.GRAPH_MIXEDNET, 31)}


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_step_by_step_equals_whole_sequence(name):
    flags, T = TOPOLOGIES[name]
    om = ec.perturbed_oracle(T, flags=flags)
    net = so.Net(flags, om)
    x = np.random.default_rng(1).uniform(0, 30, size=(3 * T + 4, 40))
    a = so.StepStream(net).run(x)
    b = so.whole_sequence(net, x)
    assert a.shape == b.shape == ((3 * T + 4) // int(flags["stride"]),)
    assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_stream_after_warm_up_equals_non_streaming_model(name):
    flags, T = TOPOLOGIES[name]
    s = int(flags["stride"])
    om = ec.perturbed_oracle(T, flags=flags)
    x = np.random.default_rng(2).uniform(0, 30, size=(2 * T + 7, 40))
    z = so.StepStream(so.Net(flags, om)).run(x)
    for n in range(len(z)):
        e = (n + 1) * s
        if e >= T:
            _, ref = om.predict_with_logits(x[None, e - T:e])
            assert abs(z[n] - ref[0]) <= 1e-12, (n, z[n], ref[0])


def test_zero_state_warm_up_differs_from_zero_frames():
    """the padding is per-layer activations, not zero spectrogram frames"""
    flags, T = TOPOLOGIES["DEF"]
    om = ec.perturbed_oracle(T, flags=flags)
    x = np.random.default_rng(3).uniform(0, 30, size=(T, 40))
    z = so.whole_sequence(so.Net(flags, om), x)
    zero_frames = om.predict_with_logits(np.concatenate([np.zeros((T - 1, 40)), x[:1]])[None])[1][0]
    assert abs(z[0] - zero_frames) > 1e-6


def test_false_accepts_per_hour_matches_fixture():
    g = np.load(GOLDEN)
    mas = [g["fa/ma%d" % i] for i in range(int(g["fa/n"]))]
    faph = streaming.false_accepts_per_hour(mas, streaming.CUTOFFS, 25, stride=2, step_s=0.02)
    assert np.abs(faph - g["fa/faph"]).max() <= 1e-12 * max(1.0, np.abs(g["fa/faph"]).max())


@pytest.mark.parametrize("case", ["busy", "quiet"])
def test_roc_matches_fixture(case, tmp_path):
    g = np.load(GOLDEN)
    probs, off, n_amb = g[case + "/probs"], g[case + "/offsets"], int(g[case + "/n_ambient"])
    tracks = [probs[off[i]:off[i + 1]] for i in range(off.size - 1)]
    r = streaming.evaluate_probabilities(tracks[:n_amb], tracks[n_amb:])
    assert np.array_equal(r["counts"].astype(np.int64), g[case + "/counts"])
    for k in ("faph", "frr", "x", "y"):
        assert r[k].shape == g[case + "/" + k].shape
        assert np.abs(r[k] - g[case + "/" + k]).max() <= 1e-12 * max(1.0, np.abs(g[case + "/" + k]).max()), k
    assert np.array_equal(r["cutoffs"], g[case + "/cut"])
    assert abs(r["auc"] - g[case + "/auc"]) <= 1e-12
    assert r["text"] == str(g[case + "/text"][()])


def test_roc_branches_covered_by_fixture():
    g = np.load(GOLDEN)
    assert g["busy/faph"][0] > 2.0 >= g["quiet/faph"][0]


def test_positive_without_moving_average_raises():
    with pytest.raises(ValueError, match="positive track 1"):
        streaming.evaluate_probabilities([np.zeros(50, np.float32)], [np.zeros(40, np.float32), np.zeros(29, np.float32)])


@pytest.mark.reference
def test_fixture_regenerates_from_reference():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_streaming_metrics as mk
    fx = mk.run_reference()
    g = np.load(GOLDEN)
    for k, v in fx.items():
        assert np.array_equal(np.asarray(v), np.asarray(g[k])), k


def _handler(tmp_path):
    from microwakeword_amd.data import FeatureHandler
    rng = np.random.default_rng(0)
    stores = {"testing": [[rng.integers(0, 900, size=(n, 40)).astype(np.uint16) for n in (5, 30, 12, 60)]],
              "testing_ambient": [[rng.integers(0, 900, size=(n, 40)).astype(np.uint16) for n in (100, 7)]]}

    class Store(list):
        pass
    cfg = {"stride": 1, "window_step_ms": 20,
           "features": [dict(type="mmap", features_dir=None, truth=True, sampling_weight=1.0, penalty_weight=1.0,
                             truncation_strategy="truncate_start", fixed_right_cutoffs=[0, 2],
                             stores={m: [Store(v) for v in s] for m, s in stores.items()}),
                        dict(type="mmap", features_dir=None, truth=False, sampling_weight=1.0, penalty_weight=2.0,
                             truncation_strategy="split", stores={"testing": [Store([rng.integers(0, 900, size=(40, 40)).astype(np.uint16)])]})]}
    return FeatureHandler(cfg), stores


def test_get_data_none_order_values_and_rng(tmp_path):
    random.seed(5)
    np.random.seed(5)
    fh, stores = _handler(tmp_path)
    py, npst = random.getstate(), np.random.get_state()
    x, y, w = fh.get_data("testing", 8, 20, truncation_strategy="none")
    assert random.getstate() == py
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:2], npst[1:2]))
    p0 = fh.feature_providers[0]
    expect = []
    for fi, sub in p0.feature_sets["testing"]:
        a = stores["testing"][0][sub].astype(np.float32) * np.float32(0.0390625)
        if a.shape[0] <= 20:
            a = np.pad(a, ((20 - a.shape[0], 0), (0, 0)))
        expect += [a, a]
    expect.append(fh.feature_providers[1].loaded_features[0][0].astype(np.float32) * np.float32(0.0390625))
    assert len(x) == len(expect) and all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(x, expect))
    assert list(y) == [1.0] * 8 + [0.0] and list(w) == [1.0] * 8 + [2.0]
