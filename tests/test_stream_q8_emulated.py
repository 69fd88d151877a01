"""The int8 streaming model (csrc/tu_stream_q8.hip) under the host-side emulator of tests/hipemu, small sizes: uint8
outputs and int8 rings equal to the NumPy restatement of tests/quant_oracle.py, stream mode equal to non_stream mode past
the warm-up, and the float kernel's range recording (mww_stream_calibrate_host) against the float stream and the float64
oracle."""
import numpy as np
import pytest

import engine_checks as ec
import q8_checks as qc
import quant_oracle as qo

# (flags, T) as in test_streaming_emulated.py
TOPOLOGIES = {"DEF": (ec.DEF, 52), "NOTEBOOK": (ec.NOTEBOOK, 164), "GRAPH_MIXEDNET": (ec.GRAPH_MIXEDNET, 31)}


@pytest.fixture(scope="module")
def quantized(emu_lib):
    cache = {}

    def get(name):
        if name not in cache:
            flags, T = TOPOLOGIES[name]
            cache[name] = qc.make_quantized(emu_lib, flags, T)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_q8_stream_matches_oracle(emu_lib, quantized, name):
    flags, T = TOPOLOGIES[name]
    s = int(flags["stride"])
    _, model, qm = quantized(name)
    # lengths not multiples of s, shorter than the receptive field, empty, padded, one spanning two 256-output tiles,
    # u16 and f32 stores; a second call continues the state of the first
    calls = [([0, 7, T + 5, 3, 300 * s + 1, 1], [0, 2, 0, 0, 4, 0]), ([2 * T + 1, 0, 5], [0, 0, 5])]
    qc.check_q8_stream_parity(emu_lib, flags, T, calls, qm=qm, model=model)


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_q8_non_stream_matches_oracle(emu_lib, quantized, name):
    flags, T = TOPOLOGIES[name]
    s = int(flags["stride"])
    _, model, qm = quantized(name)
    qc.check_q8_non_stream(emu_lib, flags, T, [T, T - 1, 0, T + 3 * s + 1, 260 * s + T], [T // 2, 0, 0, 0, 0], qm=qm, model=model)


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_q8_stream_equals_non_stream_past_warmup(emu_lib, quantized, name):
    flags, T = TOPOLOGIES[name]
    _, model, qm = quantized(name)
    qc.check_stream_equals_non_stream_past_warmup(model, qm, flags, T, [T + 40, 3 * T + 7])


def test_q8_global_scratch_form(emu_lib, quantized):
    # pointwise width 320: a 256-output tile does not fit in LDS, the kernel takes its per-workgroup global scratch
    from microwakeword_amd import streaming
    _, model, _ = quantized("DEF")
    desc = streaming.stream_description(dict(ec.DEF, pointwise_filters="64,64,64,320"), 6, 52, 1, "stream")
    qm = qc.synthetic_quantized(desc)
    qc.check_q8_stream_parity(emu_lib, ec.DEF, 52, [([300, 7, 90], [0, 2, 0]), ([60], [0])], qm=qm, model=model)


def test_step_oracle_equals_whole_sequence_oracle(emu_lib, quantized):
    for name in sorted(TOPOLOGIES):
        flags, T = TOPOLOGIES[name]
        _, _, qm = quantized(name)
        rng = np.random.default_rng(3)
        frames = rng.integers(0, 800, size=(3 * T + 2, 40)).astype(np.float32) * np.float32(0.0390625)
        step = qo.StepStreamQ8(qm)
        u8_step = step.run(frames)
        u8, _, st = qo.whole_sequence(qm, frames)
        assert np.array_equal(u8_step, u8), name
        assert np.array_equal(step.state(), st), name


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_calibration_ranges(emu_lib, name):
    flags, T = TOPOLOGIES[name]
    qc.check_calibration(emu_lib, flags, T, 3 * T + 1)


def test_predict_spectrogram_equals_predict_tracks(emu_lib, quantized):
    from microwakeword_amd import streaming
    import streaming_checks as sc
    flags, T = TOPOLOGIES["GRAPH_MIXEDNET"]
    _, model, qm = quantized("GRAPH_MIXEDNET")
    s = int(flags["stride"])
    a = streaming.QuantizedStreamingModel(qm, s, "stream", context=model)
    b = streaming.QuantizedStreamingModel(qm, s, "stream", context=model)
    tr = sc.Tracks(model, [40, 3, 77, 0, 120], seed=3)
    a.native.run(tr.win)
    whole = a.read_probabilities()
    parts = [b.predict_spectrogram(f) for f in tr.frames]
    assert np.array_equal(np.concatenate(parts), whole)
