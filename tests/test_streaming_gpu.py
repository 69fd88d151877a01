"""Streaming inference and detection metrics on the MI355X at realistic sizes (csrc/tu_stream.hip), against the float64
restatement of tests/streaming_oracle.py and the stored metric fixture."""
import os

import numpy as np
import pytest

import engine_checks as ec
import streaming_checks as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_metrics_golden.npz")


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


def _calls(T, s, rng):
    amb = [int(v) for v in rng.integers(30000, 36000, 8)]
    pos = [int(v) for v in rng.integers(60, 200, 300)] + [T - 1, 0, 3]
    return [(amb, [0] * len(amb)), (pos, [min(int(v), L) for v, L in zip(rng.integers(0, 20, len(pos)), pos)])]


@pytest.mark.parametrize("name,T", [("DEF", 194), ("NOTEBOOK", 194)])
def test_stream_parity_realistic(lib, name, T):
    flags = getattr(ec, name)
    sc.check_stream_parity(lib, flags, T, _calls(T, int(flags["stride"]), np.random.default_rng(1)))


@pytest.mark.parametrize("name,T", [("DEF", 194), ("NOTEBOOK", 194)])
def test_non_stream_parity_realistic(lib, name, T):
    flags = getattr(ec, name)
    rng = np.random.default_rng(2)
    lengths = [int(v) for v in rng.integers(1500, 2000, 4)] + [int(v) for v in rng.integers(60, 400, 200)]
    pads = [0] * 4 + [max(0, T - L) for L in lengths[4:]]
    lengths = [max(L, T) if p else L for L, p in zip(lengths, pads)]
    sc.check_non_stream_parity(lib, flags, T, lengths, pads, against_model=False)


def test_metrics_kernel_on_fixture_probabilities(lib):
    from microwakeword_amd import streaming
    g = np.load(GOLDEN)
    _, model = sc.make_model(lib, ec.DEF, 194)
    sm = streaming.StreamingModel(model, 1, "stream")
    flat, off = g["roc/probs"], g["roc/offsets"]
    n_amb = int(g["roc/n_ambient"])
    sm.native.set_probs(flat)
    kind = np.array([0] * n_amb + [1] * (off.size - 1 - n_amb), np.int32)
    counts, _, _ = sm.metrics(off, kind)
    assert np.array_equal(counts, g["roc/counts"].astype(np.uint64))
    sc.check_metrics_kernel(sm, np.random.default_rng(7), n_tracks=40, max_len=20000)


def test_bit_identical_runs(lib):
    from microwakeword_amd import streaming
    _, model = sc.make_model(lib, ec.DEF, 194)
    tr = sc.Tracks(model, [40000, 3001, 150, 20000], seed=4)
    out = []
    for _ in range(2):
        sm = streaming.StreamingModel(model, 1, "stream")
        sm.native.run(tr.win)
        out.append(sm.read_probabilities())
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


def test_predict_spectrogram_chunks_equal_predict_tracks(lib):
    sc.check_predict_spectrogram_chunks(lib, ec.NOTEBOOK, 194, [5000, 3, 190, 0, 2501])
