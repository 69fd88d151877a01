"""int8 streaming evaluation of Inception models (csrc/tu_stream_graph_q8.hip behind mww_stream_create_convnet_q8) under
the host-side emulator of tests/hipemu, small sizes, bit for bit against the NumPy restatement of
tests/quant_graph_oracle.py; the calibration pass of the float graph kernel against the float stream and float64."""
import ctypes as C

import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_checks as ic
import quant_graph_checks as gc
import quant_graph_oracle as qgo
from microwakeword_amd import native, quantize_graph, streaming

EMU = ["INC", "INC_VARIANT", "RANDOM_3"]


@pytest.mark.parametrize("name", EMU + ["FUSED_10", "FUSED_16", "RELU_ZP"])
def test_q8_stream_matches_oracle(emu_lib, name):
    # RELU_ZP: zero points above -128, where the fused ReLU's clamp to zp_out shows
    # FUSED_10: channel slices at c0 = 10 and 20 (the byte path); FUSED_16: at c0 = 16 and 32 (the word path with c0 != 0)
    gc.check_q8_stream_parity(emu_lib, gc.cases()["emu/" + name])


@pytest.mark.parametrize("name", EMU + ["FUSED_10"])
def test_q8_non_stream_matches_oracle(emu_lib, name):
    case = gc.cases()["emu/" + name]
    gc.check_q8_non_stream(emu_lib, case, *ic._emu_non_stream(case.T))


@pytest.mark.parametrize("name", ["INC_VARIANT", "FUSED_16"])
def test_q8_stream_equals_non_stream_past_warmup(emu_lib, name):
    case = gc.cases()["emu/" + name]
    gc.check_stream_equals_non_stream_past_warmup(emu_lib, case, [300, case.T + 7, 2 * case.T + 17])


def test_q8_global_scratch_form(emu_lib):
    case = gc.cases()["emu/BIG"]
    model = gc.context_model(emu_lib, case)
    st = native.GraphStream(model.engine, case.qm.desc, int8=True)
    assert st.q8_sizes() == tuple(a.size for a in case.qm.packed()[:2])
    gc.check_q8_stream_parity(emu_lib, case, model=model)


def test_q8_lds_form_above_64_kb(emu_lib):
    gc.check_q8_stream_parity(emu_lib, gc.cases()["emu/MID"])


def test_fresh_int8_streams_are_bit_equal_and_reset_restores_the_zero_points(emu_lib):
    gc.check_bit_identical(emu_lib, gc.cases()["emu/INC"], [90, 3, 280])


def test_saved_and_loaded_parameters_give_the_same_outputs_and_rings(emu_lib, tmp_path):
    case = gc.cases()["emu/INC_VARIANT"]
    path = str(tmp_path / "stream_state_internal_quant.npz")
    case.qm.save(path)
    model = gc.context_model(emu_lib, case)
    tr = ic.Tracks([130, 7], [0, 2], seed=8).upload(model)
    got = []
    for q in (case.qm, path):
        qsm = streaming.QuantizedStreamingModel(q, 1, "stream", context=model)
        qsm.native.run(tr.win)
        got.append((qsm.read_q8(), qsm.get_state_q8()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    ref = qgo.whole_sequence(quantize_graph.QuantizedGraphModel.load(path), ic.all_frames([tr]))
    assert np.array_equal(got[1][0], ref[0]) and np.array_equal(got[1][1], ref[2])


@pytest.mark.parametrize("name", EMU)
def test_calibration_ranges(emu_lib, name):
    flags, T = ic.EMU_TOPOLOGIES[name]
    gc.check_calibration(emu_lib, flags, T, 3 * T + 300)   # more than one tile


def test_calibrate_and_quantize_of_a_model(emu_lib):
    case = gc.cases()["emu/INC"]
    om, model = ic.make_model(emu_lib, case.flags, case.T)

    class Data:
        def get_data(self, mode, n, features_length):
            assert (mode, n, features_length) == ("training", 500, case.T)
            rng = np.random.default_rng(1)
            return [rng.integers(0, 900, size=(case.T, 40)).astype(np.float32) * np.float32(0.0390625) for _ in range(5)], None, None
    ranges = quantize_graph.calibrate(model, Data(), {"spectrogram_length": case.T, "stride": 1})
    frames = quantize_graph.calibration_frames(Data(), {"spectrogram_length": case.T})
    assert frames.shape == (5 * (case.T - 1), 40) and ranges[0].tolist() == [0.0, frames.max()]
    ref = gc.float64_ranges(om, case.flags, frames)
    assert np.all(np.abs(ranges - ref) <= gc.RANGE_RTOL * np.abs(ref).max(axis=1, keepdims=True))
    qm = quantize_graph.quantize(model, ranges)
    assert qm.desc == quantize_graph.QuantizedGraphModel(streaming.graph_stream_description(case.flags, case.T, 1, "stream"),
                                                         qm.scales, qm.zero_points, qm.ops, qm.lut).desc
    gc.check_q8_stream_parity(emu_lib, case, model=model, qm=qm, calls=[([70, 9], [0, 3])])


def test_creation_refuses_what_the_plain_creator_refuses(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    d = streaming.graph_stream_description(ec.INC, 60, 1, "stream")
    native.GraphStream(model.engine, d, int8=True).close()

    def with_op(i, **kw):
        ops = [dict(o) for o in d["conv_ops"]]
        ops[i].update(kw)
        return dict(d, conv_ops=ops)

    for bad, field in ((with_op(3, residual=1), "residual"), (with_op(2, kind="depthwise"), "kind"), (with_op(0, stride=2), "stride"),
                       (with_op(1, norm="bias"), "norm"), (with_op(1, act="linear"), "act"), (dict(d, head_attention=1), "head_attention"),
                       (dict(d, head_pool=2), "head_pool"), (with_op(len(d["conv_ops"]) - 1, drop=[0, 0, 0]), "src_drop"),
                       (dict(d, frames=20), "frames")):
        with pytest.raises(native.NativeError, match="error -3.*" + field):
            native.GraphStream(model.engine, bad, int8=True)


def test_a_plain_graph_stream_still_refuses_the_int8_calls_and_names_the_new_creator(emu_lib):
    _, model = ic.make_model(emu_lib, ec.INC, 60)
    st = streaming.StreamingModel(model, 1, "stream").native
    for call in (st.num_tensors, st.q8_sizes, st.get_state_q8, lambda: st.calibrate_host(np.zeros((4, 40), np.float32))):
        with pytest.raises(native.NativeError, match="MixedNet streams only.*mww_stream_create_convnet_q8"):
            call()


def test_set_quantized_validates_sizes_zero_points_and_shifts(emu_lib):
    case = gc.cases()["emu/INC"]
    model = gc.context_model(emu_lib, case)
    st = native.GraphStream(model.engine, case.qm.desc, int8=True)
    w, iv, s0, lut = case.qm.packed()
    n = len(case.qm.desc["conv_ops"])
    with pytest.raises(native.NativeError, match="no int8 parameters"):
        st.get_state_q8()
    with pytest.raises(native.NativeError, match="expected %d int8 weights and %d int32 values" % (w.size, iv.size)):
        st.set_quantized(w[:-4], iv, s0, lut)
    with pytest.raises(native.NativeError, match="expected"):
        st.set_quantized(w, iv[:-1], s0, lut)
    bad = iv.copy()
    bad[-(n + 2) + 3] = 128
    with pytest.raises(native.NativeError, match="zero points"):
        st.set_quantized(w, bad, s0, lut)
    bad = iv.copy()
    bad[2 * case.qm.desc["conv_ops"][0]["filters"]] = 31   # the first shift of op 0
    with pytest.raises(native.NativeError, match="shifts lie in"):
        st.set_quantized(w, bad, s0, lut)
    bad = iv.copy()
    bad[case.qm.desc["conv_ops"][0]["filters"]] = -1       # the first multiplier of op 0
    with pytest.raises(native.NativeError, match="multipliers"):
        st.set_quantized(w, bad, s0, lut)
    with pytest.raises(native.NativeError, match="input scale"):
        st.set_quantized(w, iv, 0.0, lut)
    with pytest.raises(native.NativeError, match="set_weights first"):
        st.run_host(np.zeros((3, 40), np.float32))
    st.set_quantized(w, iv, s0, lut)   # the stream is intact after the refusals
    assert st.run_host(np.zeros((3, 40), np.float32)) == 3 and st.read_q8().size == 3
    # the C entry point's own answer on a stream of the new creator
    r = np.zeros(2 * (n + 2), np.float32)
    rc = emu_lib.lib.mww_stream_calibrate_host(st.h, np.zeros((3, 40), np.float32).ctypes.data_as(C.POINTER(C.c_float)), 3,
                                               r.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == -4 and b"set_weights first" in emu_lib.lib.mww_last_error()   # calibration runs the float weights


@pytest.mark.parametrize("i", gc.SWEEP)
def test_q8_topology_sweep(emu_lib, i):
    gc.check_q8_stream_parity(emu_lib, gc.cases()["sweep/%d" % i])


def test_metrics_kernel_reads_the_int8_probabilities(emu_lib):
    import streaming_checks as sc
    case = gc.cases()["emu/INC"]
    model = gc.context_model(emu_lib, case)
    qsm = streaming.QuantizedStreamingModel(case.qm, 1, "stream", context=model)
    tr = ic.Tracks([90, 120, 60, 80], seed=9).upload(model)
    off = qsm.native.run(tr.win)
    sc.check_metrics_on(qsm, qsm.read_probabilities(), off, 2)
