"""Checks of the streaming evaluation of Inception models (csrc/tu_stream_graph.hip through microwakeword_amd.streaming)
shared by the emulator tests (tests/test_inception_streaming_emulated.py, small sizes), the GPU tests
(tests/test_inception_streaming_gpu.py, realistic sizes) and the input condition of both
(tests/test_inception_streaming_cpu.py).  Every check compares against the float64 restatement of
tests/inception_streaming_oracle.py; the non-stream mode against the graph oracle ``om.predict_with_logits`` itself.

Bounds: ``ec.FWD_TOL`` on logits and activation rings, ``streaming_checks.PROB_TOL`` on probabilities, exact equality on the
ring of an op fed by the spectrogram (it copies input frames).  Every case listed here is held by the CPU test to the input
condition: the float32 mode of the oracle stays within a quarter of each bound of the float64 one."""
import numpy as np

from microwakeword_amd import inception, native, streaming
import engine_checks as ec
import inception_streaming_oracle as io
from streaming_checks import PROB_TOL

CONDITION = 0.25   # share of a bound the float32 restatement may use up


def _gpu_calls(T, rng):
    """the shape of tests/test_streaming_gpu.py::_calls: eight ambient tracks, then ~300 short positives with pads"""
    amb = [int(v) for v in rng.integers(30000, 36000, 8)]
    pos = [int(v) for v in rng.integers(60, 200, 300)] + [T - 1, 0, 3]
    return [(amb, [0] * len(amb)), (pos, [min(int(v), L) for v, L in zip(rng.integers(0, 20, len(pos)), pos)])]


def _emu_calls(T):
    # empty, shorter than the receptive field, left-padded, one spanning more than one 256-output tile; a second call
    # continues the state of the first
    return [([0, 7, T + 5, 3, 301, 1], [0, 2, 0, 0, 4, 0]), ([2 * T + 1, 0, 5], [0, 0, 5])]


def _emu_non_stream(T):
    return [T, T - 1, 0, T + 4, 260 + T], [T // 2, 0, 0, 0, 0]


def _gpu_non_stream(T, rng):
    lengths = [int(v) for v in rng.integers(1500, 2000, 2)] + [int(v) for v in rng.integers(60, 400, 100)]
    pads = [0] * 2 + [max(0, T - L) for L in lengths[2:]]
    lengths, pads = [max(L, T) if p else L for L, p in zip(lengths, pads)], pads
    # unpadded tracks shorter than T (no output) between tracks that have outputs: the segment / offset tables skip them
    for at, L in ((1, T - 1), (40, 0), (41, 17), (len(lengths), T - 2)):
        lengths.insert(at, L)
        pads.insert(at, 0)
    return lengths, pads


def sweep_case(i):
    """seeded random topology i at moderate size: (flags, T, calls)"""
    flags = ec.random_inception_flags(i)
    rng = np.random.default_rng(700 + i)
    T = int(rng.integers(100, 150))
    lengths = [int(rng.integers(2000, 4000)), int(rng.integers(1, 60)), 0, int(rng.integers(300, 900))]
    pads = [0, min(3, lengths[1]), 0, 11]
    return flags, T, [(lengths, pads), ([int(rng.integers(200, 700)), 5], [0, 5])]


# twelve of the seeds 0..19 that meet the input condition (seed 10 does not: its float32 restatement uses 0.274 of PROB_TOL,
# so it is left out rather than given a looser bound); they cover two stem layers (2, 3, 4, 7, 9, 17, 19), dilation 2
# (2, 16, 18, 19) and sub-spectral groups > 1 in the stem (1, 2, 4, 6, 7, 9, 17, 18, 19) and in the blocks (2, 3, 4, 6, 12, 16, 17)
SWEEP = (1, 2, 3, 4, 6, 7, 9, 12, 16, 17, 18, 19)

EMU_TOPOLOGIES = {"INC": (ec.INC, 60), "INC_VARIANT": (ec.INC_VARIANT, 60), "RANDOM_3": (ec.random_inception_flags(3), 60)}
GPU_TOPOLOGIES = {"INC": (ec.INC, 176), "INC_VARIANT": (ec.INC_VARIANT, 150)}


def stream_cases():
    """name -> (flags, T, calls, seed) of every stream-mode case a kernel test runs"""
    out = {}
    for name, (flags, T) in EMU_TOPOLOGIES.items():
        out["emu/" + name] = (flags, T, _emu_calls(T), 0)
    for name, (flags, T) in GPU_TOPOLOGIES.items():
        out["gpu/" + name] = (flags, T, _gpu_calls(T, np.random.default_rng(1)), 0)
    for i in SWEEP:
        flags, T, calls = sweep_case(i)
        out["sweep/%d" % i] = (flags, T, calls, 50 + i)
    return out


def non_stream_cases():
    """name -> (flags, T, lengths, pads, seed)"""
    out = {}
    for name, (flags, T) in EMU_TOPOLOGIES.items():
        out["emu/" + name] = (flags, T) + _emu_non_stream(T) + (0,)
    for name, (flags, T) in GPU_TOPOLOGIES.items():
        out["gpu/" + name] = (flags, T) + _gpu_non_stream(T, np.random.default_rng(2)) + (0,)
    return out


class Tracks:
    """Synthetic tracks (even ones raw u16 micro-frontend values, odd ones float32) and, with ``upload``, two resident
    stores of ``model.engine`` holding them."""

    def __init__(self, lengths, pads=None, seed=0):
        rng = np.random.default_rng(seed)
        self.lengths = list(lengths)
        self.pads = list(pads) if pads is not None else [0] * len(self.lengths)
        u16, f32, self.rows, self.frames = [], [], [], []
        ou = of = 0
        for i, (L, pad) in enumerate(zip(self.lengths, self.pads)):
            rows = L - pad
            if i % 2 == 0:
                raw = rng.integers(0, 1200, size=(rows, 40)).astype(np.uint16)
                u16.append(raw.reshape(-1))
                self.rows.append((0, pad, rows, 0, ou))
                ou += raw.size
                x = raw.astype(np.float32) * np.float32(0.0390625)
            else:
                x = rng.uniform(0, 40, size=(rows, 40)).astype(np.float32)
                f32.append(x.reshape(-1))
                self.rows.append((1, pad, rows, 0, of))
                of += x.size
            self.frames.append(np.concatenate([np.zeros((pad, 40), np.float32), x], 0))
        self.u16 = np.concatenate(u16 + [np.zeros(40, np.uint16)])
        self.f32 = np.concatenate(f32 + [np.zeros(40, np.float32)])

    def upload(self, model, store_ids=(0, 1)):
        model.engine.upload_store(store_ids[0], self.u16)
        model.engine.upload_store(store_ids[1], self.f32)
        self.win = np.array([(store_ids[r[0]],) + r[1:] for r in self.rows], native.WINDOW_DTYPE).reshape(-1)
        return self


def cli_config(tmp_path, T):
    """a tiny test configuration for model_train_eval.evaluate_model: 6 positives long enough for 30 non-streaming windows,
    4 negatives, 2 ambient tracks"""
    rng = np.random.default_rng(0)

    def samples(n, lo, hi):
        return [[rng.integers(0, 900, size=(int(rng.integers(lo, hi)), 40)).astype(np.uint16) for _ in range(n)]]
    pos = {"testing": samples(6, T + 40, T + 80)}
    neg = {"testing": samples(4, T, T + 30), "testing_ambient": samples(2, 3 * T, 4 * T)}
    return {"stride": 1, "window_step_ms": 20, "train_dir": str(tmp_path / "run"), "batch_size": 8, "spectrogram_length": T,
            "training_input_shape": (T, 40),
            "features": [dict(type="mmap", stores=pos, truth=True, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
                         dict(type="mmap", stores=neg, truth=False, sampling_weight=1.0, penalty_weight=1.0, truncation_strategy="split")]}


def make_model(lib, flags, T, seed=42):
    om = ec.perturbed_inception_oracle(T, flags, seed=seed)
    model = inception.model(flags, (T, 40), 4, lib=lib, max_batch=64)
    model.set_weights(om.get_weights())
    return om, model


def all_frames(tracks_list):
    fs = [f for tr in tracks_list for f in tr.frames]
    return np.concatenate(fs + [np.zeros((0, 40), np.float32)], 0)


def _compare(got_p, got_z, ref_z, what):
    ref_z = np.asarray(ref_z, np.float64)
    assert got_p.shape == ref_z.shape, (what, got_p.shape, ref_z.shape)
    if ref_z.size:
        ez, ep = np.abs(got_z - ref_z).max(), np.abs(got_p - io.sigmoid(ref_z)).max()
        print("%s: logit error %.3g (bound %g), probability error %.3g (bound %g)" % (what, ez, ec.FWD_TOL, ep, PROB_TOL))
        assert ez <= ec.FWD_TOL, (what, ez)
        assert ep <= PROB_TOL, (what, ep)


def compare_state(got, ref, net, what):
    """``mww_stream_get_state`` against the oracle's rings: stem 0's ring is a copy of input frames (exact), every other
    ring holds activations (FWD_TOL)"""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    at = 0
    for i, (name, rows, c) in enumerate(net.ring_shapes()):
        g, r = got[at:at + rows * c], ref[at:at + rows * c]
        if i == 0:
            assert np.array_equal(g, r.astype(np.float32)), (what, "ring of " + name + " (input frames) differs")
        elif g.size:
            e = float(np.abs(g - r).max())
            assert e <= ec.FWD_TOL, (what, "ring of " + name, e)
        at += rows * c
    assert at == got.size


def check_stream_parity(lib, flags, T, calls, seed=0, model_seed=42):
    """``calls``: list of (lengths, pads) run as successive mww_stream_run calls on one stream (state carried): logits,
    probabilities and the rings after every call against the oracle fed the same frames from zero state."""
    om, model = make_model(lib, flags, T, model_seed)
    sm = streaming.StreamingModel(model, 1, "stream")
    net = io.Net(flags, om)
    assert sm.native.n_state == net.n_state()
    assert np.array_equal(sm.native.get_state(), np.zeros(net.n_state(), np.float32))
    done, got = [], []
    for ci, (lengths, pads) in enumerate(calls):
        tr = Tracks(lengths, pads, seed=seed + ci).upload(model, (2 * ci, 2 * ci + 1))
        off = sm.native.run(tr.win)
        p, z = sm.native.read(want_logits=True)
        assert off[-1] == p.size and list(np.diff(off)) == list(lengths)
        got += [p, z]
        done.append(tr)
        ref_z, ref_state = io.whole_sequence(net, all_frames(done), rings=True)
        compare_state(sm.native.get_state(), ref_state, net, "state after call %d" % ci)
    at = 0
    for ci in range(len(calls)):
        n = got[2 * ci].size
        _compare(got[2 * ci], got[2 * ci + 1], ref_z[at:at + n], "call %d" % ci)
        at += n
    return om, model, sm


def check_non_stream_parity(lib, flags, T, lengths, pads, seed=0, against_model=True):
    om, model = make_model(lib, flags, T)
    sm = streaming.StreamingModel(model, 1, "non_stream")
    tr = Tracks(lengths, pads, seed=seed).upload(model)
    off = sm.native.run(tr.win)
    p, z = sm.native.read(want_logits=True)
    refs = [io.non_stream_windows(om, f, T) for f in tr.frames]
    assert list(np.diff(off)) == [r.size for r in refs] == [max(0, L - T + 1) for L in lengths]
    _compare(p, z, np.concatenate(refs + [np.zeros(0)]), "non-stream windows")
    if against_model:   # the training engine's own inference forward on the same windows
        for t, f in enumerate(tr.frames):
            if refs[t].size:
                x = np.stack([f[e - T:e] for e in range(T, len(f) + 1)])
                pm = np.concatenate([model.predict_on_batch(x[a:a + 64]).reshape(-1) for a in range(0, len(x), 64)])
                assert np.abs(pm - p[off[t]:off[t + 1]]).max() <= PROB_TOL
    return sm


def check_predict_spectrogram_chunks(lib, flags, T, lengths, seed=3):
    """StreamingModel.predict_spectrogram track by track (host frames) is bit-equal to one run over the same tracks"""
    om, model = make_model(lib, flags, T)
    a = streaming.StreamingModel(model, 1, "stream")
    b = streaming.StreamingModel(model, 1, "stream")
    tr = Tracks(lengths, seed=seed).upload(model)
    off = a.native.run(tr.win)
    whole = a.read_probabilities()
    parts = [b.predict_spectrogram(f) for f in tr.frames]
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    assert all(parts[i].size == off[i + 1] - off[i] for i in range(len(parts)))
    assert np.array_equal(a.native.get_state().view(np.uint32), b.native.get_state().view(np.uint32))
    return whole


def check_bit_identical_and_reset(lib, flags, T, lengths, seed=4):
    """two fresh streams agree bit for bit; reset() restores the zero state, after which the same run repeats itself"""
    _, model = make_model(lib, flags, T)
    tr = Tracks(lengths, seed=seed).upload(model)
    out = []
    for _ in range(2):
        sm = streaming.StreamingModel(model, 1, "stream")
        sm.native.run(tr.win)
        out.append((sm.read_probabilities(), sm.native.get_state()))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    assert np.any(out[1][1] != 0)
    sm.reset()
    assert np.array_equal(sm.native.get_state(), np.zeros(sm.native.n_state, np.float32))
    sm.native.run(tr.win)
    assert np.array_equal(sm.read_probabilities().view(np.uint32), out[0][0].view(np.uint32))
    return sm
