"""The int8 streaming model on the MI355X at realistic sizes (csrc/tu_stream_q8.hip): bit for bit against the NumPy
restatement of tests/quant_oracle.py, bit-identical reruns, stream against non_stream mode, the calibration against the
float stream and the float64 oracle, and a saved .npz reproducing the outputs."""
import numpy as np
import pytest

import engine_checks as ec
import q8_checks as qc
import streaming_checks as sc

pytestmark = pytest.mark.gpu

WIDE = dict(ec.DEF, pointwise_filters="64,64,64,320")   # a tile too large for LDS: the global-scratch form


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


def _calls(T, rng):
    amb = [int(v) for v in rng.integers(30000, 36000, 8)]
    pos = [int(v) for v in rng.integers(60, 200, 300)] + [T - 1, 0, 3]
    return [(amb, [0] * len(amb)), (pos, [min(int(v), L) for v, L in zip(rng.integers(0, 20, len(pos)), pos)])]


@pytest.mark.parametrize("name,T", [("DEF", 194), ("NOTEBOOK", 194)])
def test_q8_stream_parity_realistic(lib, name, T):
    flags = getattr(ec, name)
    qc.check_q8_stream_parity(lib, flags, T, _calls(T, np.random.default_rng(1)))


def test_q8_global_scratch_form(lib):
    from microwakeword_amd import streaming
    _, model = sc.make_model(lib, ec.DEF, 52)
    qm = qc.synthetic_quantized(streaming.stream_description(WIDE, 6, 52, 1, "stream"))
    qc.check_q8_stream_parity(lib, ec.DEF, 52, [([30000, 7, 900], [0, 2, 0]), ([1200], [0])], qm=qm, model=model)


def test_q8_bit_identical_reruns(lib):
    from microwakeword_amd import streaming
    _, model, qm = qc.make_quantized(lib, ec.DEF, 194)
    tr = sc.Tracks(model, [40000, 3001, 150, 20000], seed=4)
    out = []
    for _ in range(2):
        qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
        qsm.native.run(tr.win)
        out.append((qsm.read_q8(), qsm.get_state_q8(), qsm.read_probabilities()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2].view(np.uint32), out[1][2].view(np.uint32))


@pytest.mark.parametrize("name,T", [("DEF", 194), ("NOTEBOOK", 194)])
def test_q8_stream_equals_non_stream(lib, name, T):
    flags = getattr(ec, name)
    _, model, qm = qc.make_quantized(lib, flags, T)
    qc.check_stream_equals_non_stream_past_warmup(model, qm, flags, T, [5000, T + 7, 2 * T + 17])
    qc.check_q8_non_stream(lib, flags, T, [1800, T, 300], [0, 20, 0], qm=qm, model=model)


@pytest.mark.parametrize("name,T", [("DEF", 194), ("NOTEBOOK", 194)])
def test_calibration_consistency(lib, name, T):
    qc.check_calibration(lib, getattr(ec, name), T, 20000)


def test_loaded_npz_reproduces_the_outputs(lib, tmp_path):
    from microwakeword_amd import streaming
    _, model, qm = qc.make_quantized(lib, ec.NOTEBOOK, 194)
    path = str(tmp_path / "stream_state_internal_quant.npz")
    qm.save(path)
    tr = sc.Tracks(model, [9000, 400, 2000], seed=6)
    a = streaming.QuantizedStreamingModel(qm, 3, "stream", context=model)
    b = streaming.QuantizedStreamingModel(path, 3, "stream", context=model)
    oa, ob = a.native.run(tr.win), b.native.run(tr.win)
    assert np.array_equal(oa, ob)
    assert np.array_equal(a.read_q8(), b.read_q8()) and np.array_equal(a.get_state_q8(), b.get_state_q8())
