"""Streaming / non-streaming evaluation of Inception models (csrc/tu_stream_graph.hip) under the host-side emulator of
tests/hipemu, small sizes, against the float64 restatement of tests/inception_streaming_oracle.py and the graph oracle."""
import ctypes as C

import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_checks as ic
import streaming_checks as sc
from microwakeword_amd import native, quantize, streaming


@pytest.mark.parametrize("name", sorted(ic.EMU_TOPOLOGIES))
def test_stream_mode_matches_oracle(emu_lib, name):
    flags, T, calls, seed = ic.stream_cases()["emu/" + name]
    ic.check_stream_parity(emu_lib, flags, T, calls, seed)


@pytest.mark.parametrize("name", sorted(ic.EMU_TOPOLOGIES))
def test_non_stream_mode_matches_graph_oracle_and_model(emu_lib, name):
    flags, T, lengths, pads, seed = ic.non_stream_cases()["emu/" + name]
    ic.check_non_stream_parity(emu_lib, flags, T, lengths, pads, seed)


def test_predict_spectrogram_track_by_track_equals_one_run(emu_lib):
    ic.check_predict_spectrogram_chunks(emu_lib, ec.INC_VARIANT, 60, [40, 3, 77, 0, 300])


def test_fresh_streams_are_bit_equal_and_reset_restores_zero_state(emu_lib):
    ic.check_bit_identical_and_reset(emu_lib, ec.INC, 60, [90, 3, 280])


def test_metrics_kernel_on_the_kernels_own_probabilities(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    sm = streaming.StreamingModel(model, 1, "stream")
    tr = ic.Tracks([90, 120, 60, 80], seed=9).upload(model)
    off = sm.native.run(tr.win)
    sc.check_metrics_on(sm, sm.read_probabilities(), off, 2)


def test_stride_other_than_one_is_refused(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    with pytest.raises(ValueError, match="stride \\(3\\)"):
        streaming.StreamingModel(model, 3, "stream")
    with pytest.raises(ValueError, match="mode"):
        streaming.StreamingModel(model, 1, "tflite")


def test_descriptions_outside_the_vocabulary_are_refused(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    d = streaming.graph_stream_description(ec.INC, 60, 1, "stream")
    native.GraphStream(model.engine, d).close()

    def with_op(i, **kw):
        ops = [dict(o) for o in d["conv_ops"]]
        ops[i].update(kw)
        return dict(d, conv_ops=ops)

    for bad, field in ((with_op(3, residual=1), "residual"), (with_op(2, kind="depthwise"), "kind"), (with_op(0, stride=2), "stride"),
                       (with_op(1, norm="bias"), "norm"), (with_op(1, act="linear"), "act"), (dict(d, head_attention=1), "head_attention"),
                       (dict(d, head_pool=2), "head_pool"), (with_op(len(d["conv_ops"]) - 1, drop=[0, 0, 0]), "src_drop"),
                       (dict(d, frames=20), "frames")):
        with pytest.raises(native.NativeError, match="error -3.*" + field):
            native.GraphStream(model.engine, bad)


def test_int8_entry_points_refuse_a_graph_stream(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    sm = streaming.StreamingModel(model, 1, "stream")
    st = sm.native
    frames = np.zeros((10, 40), np.float32)
    for call in (st.num_tensors, lambda: st.calibrate_host(frames), st.q8_sizes,
                 lambda: st.set_quantized(np.zeros(4, np.int8), np.zeros(4, np.int32), 1.0, np.zeros(256, np.uint8)),
                 lambda: st.read_q8(0), st.get_state_q8):
        with pytest.raises(native.NativeError, match="MixedNet streams only"):
            call()
    # the C entry point itself, past the Python wrapper's own num_tensors call
    r = np.zeros(64, np.float32)
    rc = emu_lib.lib.mww_stream_calibrate_host(st.h, frames.ctypes.data_as(C.POINTER(C.c_float)), 10, r.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == -3 and b"MixedNet" in emu_lib.lib.mww_last_error()
    # the stream still works afterwards
    assert st.run_host(frames) == 10


def test_int8_quantization_of_an_inception_model_is_refused_before_any_kernel(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    with pytest.raises(NotImplementedError, match="int8 evaluation covers MixedNet only"):
        quantize.calibrate(model, None, {"stride": 1})
    with pytest.raises(NotImplementedError, match="int8 evaluation covers MixedNet only"):
        quantize.quantize(model, np.zeros((3, 2), np.float32))
