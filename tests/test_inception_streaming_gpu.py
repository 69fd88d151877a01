"""Streaming / non-streaming evaluation of Inception models on the MI355X at realistic sizes (csrc/tu_stream_graph.hip),
against the float64 restatement of tests/inception_streaming_oracle.py (evaluated without the [n, C, T_f] window tensor)
and the graph oracle.  Every case is listed in tests/inception_streaming_checks.py, where the CPU suite holds it to the
input condition."""
import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_checks as ic
import streaming_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_stream_parity_realistic(lib, name):
    flags, T, calls, seed = ic.stream_cases()["gpu/" + name]
    _, _, sm = ic.check_stream_parity(lib, flags, T, calls, seed)
    # the metrics kernel on the positives' probabilities of the last call
    off = np.concatenate([[0], np.cumsum(calls[-1][0])]).astype(np.int64)
    sc.check_metrics_on(sm, sm.read_probabilities(), off, 40)


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_non_stream_parity_realistic(lib, name):
    flags, T, lengths, pads, seed = ic.non_stream_cases()["gpu/" + name]
    ic.check_non_stream_parity(lib, flags, T, lengths, pads, seed, against_model=False)


@pytest.mark.parametrize("case", ic.SWEEP)
def test_topology_sweep(lib, case):
    flags, T, calls = ic.sweep_case(case)
    try:
        ic.check_stream_parity(lib, flags, T, calls, seed=50 + case)
    except AssertionError as e:
        raise AssertionError("case %d %s T=%d: %s" % (case, flags, T, e))


def test_bit_identical_runs_and_reset(lib):
    ic.check_bit_identical_and_reset(lib, ec.INC, 176, [40000, 3001, 150, 20000])


def test_predict_spectrogram_chunks_equal_predict_tracks(lib):
    ic.check_predict_spectrogram_chunks(lib, ec.INC_VARIANT, 150, [5000, 3, 190, 0, 2501])
