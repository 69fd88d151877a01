"""Streaming inference and detection metrics (csrc/tu_stream.hip) under the host-side emulator of tests/hipemu, small
sizes, against the float64 restatement of tests/streaming_oracle.py."""
import numpy as np
import pytest

import engine_checks as ec
import streaming_checks as sc

# (flags, T): T - k1 divisible by the stride, small final maps
TOPOLOGIES = {"DEF": (ec.DEF, 52), "NOTEBOOK": (ec.NOTEBOOK, 164), "GRAPH_MIXEDNET": (ec.GRAPH_MIXEDNET, 31)}


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_stream_mode_matches_oracle(emu_lib, name):
    flags, T = TOPOLOGIES[name]
    s = int(flags["stride"])
    # lengths not multiples of s, shorter than the receptive field, empty, padded, one spanning two 256-output tiles;
    # a second call continues the state of the first
    calls = [([0, 7, T + 5, 3, 300 * s + 1, 1], [0, 2, 0, 0, 4, 0]), ([2 * T + 1, 0, 5], [0, 0, 5])]
    sc.check_stream_parity(emu_lib, flags, T, calls)


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_non_stream_mode_matches_oracle_and_model(emu_lib, name):
    flags, T = TOPOLOGIES[name]
    s = int(flags["stride"])
    sc.check_non_stream_parity(emu_lib, flags, T, [T, T - 1, 0, T + 3 * s + 1, 260 * s + T], [T // 2, 0, 0, 0, 0])


def test_metrics_kernel_matches_host_restatement(emu_lib):
    flags, T = TOPOLOGIES["DEF"]
    _, model = sc.make_model(emu_lib, flags, T)
    sm = sc.streaming.StreamingModel(model, 1, "stream")
    sc.check_metrics_kernel(sm, np.random.default_rng(5))
    # on the kernel's own probabilities
    tr = sc.Tracks(model, [90, 120, 60, 80], seed=9)
    off = sm.native.run(tr.win)
    sc.check_metrics_on(sm, sm.read_probabilities(), off, 2)


def test_predict_spectrogram_chunks_equal_one_call(emu_lib):
    flags, T = TOPOLOGIES["GRAPH_MIXEDNET"]
    sc.check_predict_spectrogram_chunks(emu_lib, flags, T, [40, 3, 77, 0, 120])


def test_unsupported_topologies_are_refused(emu_lib):
    from microwakeword_amd import native, streaming
    flags, T = TOPOLOGIES["DEF"]
    _, model = sc.make_model(emu_lib, flags, T)
    with pytest.raises(NotImplementedError, match="residual_connection"):
        streaming.stream_description(dict(flags, residual_connection="1,0,0,0"), 5, T, 1, "stream")
    with pytest.raises(NotImplementedError, match="spatial_attention"):
        streaming.stream_description(dict(flags, spatial_attention=1), 5, T, 1, "stream")
    with pytest.raises(NotImplementedError, match="first_conv_filters"):
        streaming.stream_description(dict(flags, first_conv_filters=0), 5, T, 1, "stream")
    tf = model.layout.t_last
    d = streaming.stream_description(flags, tf, T, 1, "non_stream")
    native.Stream(model.engine, d).close()
    with pytest.raises(native.NativeError, match="error -3"):
        native.Stream(model.engine, dict(d, t_final=tf + 1))   # does not match the window
    with pytest.raises(native.NativeError, match="error -3"):
        native.Stream(model.engine, dict(d, blocks=[(1, (9, 5), 48)] + d["blocks"][1:]))   # kernels not ascending
