"""int8 streaming evaluation of Inception models on the MI355X (csrc/tu_stream_graph_q8.hip), bit for bit against the NumPy
restatement of tests/quant_graph_oracle.py.  Every case is listed in tests/quant_graph_checks.py, where the CPU suite
holds it to the input condition.  The first call of the two realistic cases has more than 2 x 256 tiles, so a workgroup's
tile loop runs more than once; the default flags' tile lives in LDS, MID's in LDS above 64 KB, BIG's in the global scratch."""
import numpy as np
import pytest

import inception_streaming_checks as ic
import quant_graph_checks as gc
import streaming_checks as sc
from microwakeword_amd import streaming

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_q8_stream_parity_realistic(lib, name):
    case = gc.cases()["gpu/" + name]
    assert sum(case.calls[0][0]) > 2 * 256 * 256
    gc.check_q8_stream_parity(lib, case)


@pytest.mark.parametrize("name", ["FUSED_10", "FUSED_16", "BIG", "MID", "RELU_ZP"])
def test_q8_hand_made_descriptions(lib, name):
    gc.check_q8_stream_parity(lib, gc.cases()["emu/" + name])


@pytest.mark.parametrize("i", gc.SWEEP)
def test_q8_topology_sweep(lib, i):
    gc.check_q8_stream_parity(lib, gc.cases()["sweep/%d" % i])


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_q8_non_stream_parity(lib, name):
    case = gc.cases()["gpu/" + name]
    T = case.T
    gc.check_q8_non_stream(lib, case, [T, T - 1, 0, T + 4, 700 + T, 17], [T // 2, 0, 0, 0, 0, 0])


def test_q8_runs_are_bit_identical_and_reset_restores_the_zero_points(lib):
    gc.check_bit_identical(lib, gc.cases()["gpu/INC"], [20000, 3001, 150])


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_q8_stream_equals_non_stream_past_warmup(lib, name):
    case = gc.cases()["gpu/" + name]
    gc.check_stream_equals_non_stream_past_warmup(lib, case, [5000, case.T + 7, 2 * case.T + 17])


@pytest.mark.parametrize("name", sorted(ic.GPU_TOPOLOGIES))
def test_calibration_is_consistent_with_the_float_stream_and_float64(lib, name):
    flags, T = ic.GPU_TOPOLOGIES[name]
    gc.check_calibration(lib, flags, T, 20000)


def test_metrics_kernel_reads_the_int8_probabilities(lib):
    case = gc.cases()["emu/INC"]
    model = gc.context_model(lib, case)
    qsm = streaming.QuantizedStreamingModel(case.qm, 1, "stream", context=model)
    tr = ic.Tracks([90, 120, 60, 80], seed=9).upload(model)
    off = qsm.native.run(tr.win)
    sc.check_metrics_on(qsm, qsm.read_probabilities(), off, 2)
