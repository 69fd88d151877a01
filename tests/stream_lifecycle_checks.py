"""The life of the int8 part of a stream, shared by tests/test_stream_lifecycle_emulated.py and its GPU twin: the host path
of csrc/tu_stream.hip serves MixedNet and conv/BN graph streams alike, so each check runs on one stream of either kind -
the cheapest case of ``stream_sweep.emulator_slice()`` and the smallest ``emu/`` case of ``quant_graph_checks.cases()``.
Every comparison is exact (``np.array_equal``): both sides are the same kernel on the same inputs."""
import functools

import numpy as np

import quant_graph_checks as gc
import stream_sweep as sw
import streaming_checks as sc
from microwakeword_amd import native, quantize, quantize_graph, streaming

KINDS = ("mixednet", "graph")
FRAMES = 300   # outputs of a run: more than one 256-output tile


def _graph_macs(case):
    desc = case._desc or streaming.graph_stream_description(case.flags, case.T, 1, "stream")
    ch, n = [], 0
    for o in desc["conv_ops"]:
        cin = sum((cn or (40 if s < 0 else ch[s]) - c0) for s, (c0, cn) in zip(o["src"], o["slice"]))
        n += int(o["kernel"]) * cin * int(o["filters"])
        ch.append(int(o["filters"]))
    return n


@functools.lru_cache(maxsize=None)
def setup(kind):
    """(description, Keras-order floats, two int8 parameter sets of different ranges, frames per output)"""
    if kind == "mixednet":
        b = sw.built(sw.emulator_slice()[0].id)
        desc, flat, qm, stride = b.desc, b.flat, b.qm, b.s
        other = quantize.quantize_weights(desc, b.weights, qm.ranges * np.float32(0.75))
    else:
        case = min((c for name, c in gc.cases().items() if name.startswith("emu/")), key=_graph_macs)
        desc, w, qm, _ = case.build()
        flat, stride = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in w]), 1
        other = quantize_graph.quantize_weights(desc, w, qm.ranges * np.float32(0.75))
    assert not np.array_equal(other.packed()[1], qm.packed()[1])
    return desc, flat, other, qm, stride


def _stream(lib, kind, desc):
    engine = sc.context_model(lib).engine
    return native.Stream(engine, desc) if kind == "mixednet" else native.GraphStream(engine, desc, int8=True)


def _run_q8(st, frames):
    """two calls, the second from the rings of the first: (uint8 outputs, final int8 state)"""
    half = len(frames) // 2
    out = []
    for x in (frames[:half], frames[half:]):
        st.run_host(x)
        out.append(st.read_q8())
    return np.concatenate(out), st.get_state_q8()


def check_second_parameter_set_equals_a_fresh_stream(lib, kind):
    """set_quantized, a run, set_quantized with other parameters, reset, a run == a fresh stream given the second set"""
    desc, _, first, second, stride = setup(kind)
    frames = sw.gen_frames(np.random.default_rng(5), FRAMES * stride)
    st = _stream(lib, kind, desc)
    st.set_quantized(*first.packed())
    st.run_host(frames[:(FRAMES // 3) * stride])   # leaves the rings of the first set behind, in the other half of the state
    st.set_quantized(*second.packed())
    st.reset()
    got = _run_q8(st, frames)
    st.close()
    fresh = _stream(lib, kind, desc)
    fresh.set_quantized(*second.packed())
    want = _run_q8(fresh, frames)
    fresh.close()
    assert got[0].size == FRAMES and np.unique(got[0]).size > 1
    assert np.array_equal(got[0], want[0]), "%d of %d uint8 outputs differ" % (int(np.sum(got[0] != want[0])), FRAMES)
    assert np.array_equal(got[1], want[1]), "int8 state differs"


def check_calibration_after_set_quantized_runs_the_float_kernel(lib, kind):
    """calibrate_host after set_quantized: the ranges, probabilities and float state of the float kernel, as before it"""
    desc, flat, _, qm, stride = setup(kind)
    frames = sw.gen_frames(np.random.default_rng(6), FRAMES * stride)
    st = _stream(lib, kind, desc)
    st.set_weights(flat)
    before = st.calibrate_host(frames), st.read(want_logits=True), st.get_state()
    st.reset()
    st.set_quantized(*qm.packed())
    after = st.calibrate_host(frames), st.read(want_logits=True), st.get_state()
    assert np.array_equal(before[0], after[0]) and np.all(np.isfinite(after[0])) and after[0].shape == (st.num_tensors(), 2)
    for x, y in ((before[1][0], after[1][0]), (before[1][1], after[1][1]), (before[2], after[2])):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    st.run_host(frames)   # and a run is the int8 kernel's again: probabilities u8 / 255
    assert np.array_equal(st.read().view(np.uint32), (st.read_q8().astype(np.float32) * np.float32(1.0 / 255.0)).view(np.uint32))
    st.close()
