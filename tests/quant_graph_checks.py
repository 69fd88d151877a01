"""Checks of the int8 streaming evaluation of Inception models (csrc/tu_stream_graph_q8.hip through
microwakeword_amd.quantize_graph / streaming) shared by the emulator tests (tests/test_inception_q8_emulated.py, small
sizes), the GPU tests (tests/test_inception_q8_gpu.py) and the input condition of both (tests/test_inception_q8_cpu.py).
The kernel is held bit for bit to tests/quant_graph_oracle.py (``np.array_equal``: it is an integer function of input and
parameters, so there is no tolerance); the calibration to the float graph stream and a float64 restatement.

Every case's int8 model is derived without any kernel - the calibrated ranges are those of the float64 restatement on the
case's calibration frames - so the CPU test can evaluate the input condition (``q8_checks.SPREAD_*``) of exactly the models
and frames the kernel tests run."""
import functools

import numpy as np

from microwakeword_amd import native, quantize_graph, streaming
from microwakeword_amd.layout import InceptionLayout
import engine_checks as ec
import inception_streaming_checks as ic
import inception_streaming_oracle as io
import q8_checks as qc
import quant_graph_oracle as qgo

RANGE_RTOL = qc.RANGE_RTOL


# ------------------------------------------------------------------------------------------------------------ ranges

def float64_ranges(om, flags, frames):
    """[min, max] of every tensor (input, every op in Keras layer-creation order, logit) of the float64 streaming oracle
    (inception_streaming_oracle.Net) over ``frames`` from zero state"""
    net = io.Net(flags, om)
    x = np.asarray(frames, np.float64).reshape(-1, 40)
    N = x.shape[0]
    out = [(x.min(), x.max())]

    def pad(a, rows):
        return np.concatenate([np.zeros((rows, a.shape[1])), a], 0)

    def rec(a):
        out.append((a.min(), a.max()))
        return a

    for i, (k, g) in enumerate(net.stem):
        x = rec(net.conv("stem%d" % i, g, pad(x, k - 1)))
    for i, (k, g, d) in enumerate(net.blocks):
        p, R = "i%d." % i, d * (k - 1)
        b1 = rec(net.conv(p + "b1", g, x))
        b2a = rec(net.conv(p + "b2a", g, x))
        b2 = rec(net.conv(p + "b2b", g, pad(b2a, R), d))
        b3a = rec(net.conv(p + "b3a", g, x))
        b3b = rec(net.conv(p + "b3b", g, pad(b3a, R), d))
        b3 = rec(net.conv(p + "b3c", g, pad(b3b, R), d))
        x = rec(net.conv(p + "red", 1, np.concatenate([b1, b2, b3], 1)))
    z = io.whole_sequence(net, np.asarray(frames, np.float64))
    assert z.size == N
    out.append((z.min(), z.max()))
    return np.array(out, np.float64)


def desc_ranges(desc, weights, frames):
    """the same for any graph description and its Keras-order weights (folded as quantize_graph folds them, then float64)"""
    srcs = quantize_graph.op_sources(desc)
    x = np.asarray(frames, np.float64).reshape(-1, 40)
    tensors, out, it = [x], [(x.min(), x.max())], iter(weights)
    for o, ss in zip(desc["conv_ops"], srcs):
        cin = sum(cn for _, _, cn in ss)
        w, b = quantize_graph.fold_op(o, cin, *(next(it) for _ in range(5)))
        k, d = int(o["kernel"]), int(o.get("dilation", 1))
        a = np.concatenate([tensors[t][:, c0:c0 + cn] for t, c0, cn in ss], 1)
        a = np.concatenate([np.zeros((d * (k - 1), cin)), a], 0)
        y = np.zeros((x.shape[0], w.shape[2])) + b.astype(np.float64)
        for j in range(k):
            y = y + a[j * d:j * d + x.shape[0]] @ w[j].astype(np.float64)
        tensors.append(np.maximum(y, 0))
        out.append((tensors[-1].min(), tensors[-1].max()))
    dk, db = np.asarray(next(it), np.float64).reshape(-1), float(np.asarray(next(it)).reshape(-1)[0])
    c = tensors[-1].shape[1]
    tf = dk.size // c
    h = np.concatenate([np.zeros((tf - 1, c)), tensors[-1]], 0)
    z = np.full(x.shape[0], db)
    for t in range(tf):
        z = z + h[t:t + x.shape[0]] @ dk.reshape(tf, c)[t]
    out.append((z.min(), z.max()))
    return np.array(out, np.float64)


# ------------------------------------------------------------------------------------------------------------- cases

def fused_description(f1, T):
    """hand-made: the default Inception with two blocks whose three 1x1 branch heads run as ONE op of 3 * f1 filters that the
    branches read through channel slices at c0 = f1 and 2 * f1 (InceptionLayout(fuse_heads=True), which no streaming float
    model uses): f1 = 10 puts the slices off the word grid (byte path), f1 = 16 on it (word path with c0 != 0)"""
    flags = dict(ec.INC, cnn2_filters1="%d,%d" % (f1, f1), cnn2_filters2="10,12", cnn2_kernel_sizes="5,3",
                 cnn2_subspectral_groups="1,1", cnn2_dilation="1,2")
    lay = InceptionLayout(flags, T, fuse_heads=True)
    assert any(c0 for op in lay.ops for c0, _ in op["slice"])
    return dict(conv_ops=lay.ops, op_names=lay.op_names, frames=int(T), stride=1, mode="stream")


def big_description(T, width=256):
    """hand-made: two wide ops and a concatenation of both.  At width 256 the int8 tile (256 + 59 rows of 40 + 256 + 256 + 64
    bytes: 190 KB) exceeds the 160 KB of LDS, so the kernel takes the global-scratch form; at width 128 it is 110 KB: dynamic
    LDS above the 64 KB a launch gets without raising the kernel's limit"""
    ops = [dict(src=[-1], drop=[0], slice=[(0, 0)], kernel=3, dilation=1, filters=width, bn_groups=4),
           dict(src=[0], drop=[0], slice=[(0, 0)], kernel=3, dilation=1, filters=width, bn_groups=1),
           dict(src=[0, 1], drop=[2, 0], slice=[(0, 0), (0, 0)], kernel=1, dilation=1, filters=62, bn_groups=1)]
    return dict(conv_ops=ops, op_names=["stem0", "wide", "cat"], frames=int(T), stride=1, mode="stream")


CAL_FRAMES = 400


class Case:
    """one int8 model and the stream-mode calls it is run on; ``flags`` is None for a hand-made description"""

    def __init__(self, name, T, calls, flags=None, desc=None, seed=0, model_seed=42, cal_seed=11, range_edit=None):
        self.name, self.T, self.calls, self.flags, self._desc = name, T, calls, flags, desc
        self.seed, self.model_seed, self.cal_seed, self.range_edit = seed, model_seed, cal_seed, range_edit

    @functools.lru_cache(maxsize=None)
    def build(self):
        """(description, Keras-order weights, QuantizedGraphModel, oracle model or None) - no kernel involved"""
        cal = qc.calibration_set(CAL_FRAMES, self.cal_seed)
        if self.flags is not None:
            om = ec.perturbed_inception_oracle(self.T, self.flags, seed=self.model_seed)
            desc = streaming.graph_stream_description(self.flags, self.T, 1, "stream")
            w = om.get_weights()
            ranges = float64_ranges(om, self.flags, cal)
        else:
            om, desc = None, self._desc
            w = qgo.random_weights(desc, self.model_seed)
            rng = np.random.default_rng(self.model_seed + 1000)
            c_last = int(desc["conv_ops"][-1]["filters"])
            w += [rng.normal(0, 0.05, (qgo.final_frames(desc) * c_last, 1)), rng.normal(0, 0.1, 1)]
            ranges = desc_ranges(desc, w, cal)
        if self.range_edit is not None:   # hand-set ranges, as a hand-made .npz may hold: the oracle follows whatever they say
            ranges = self.range_edit(ranges.copy())
        return desc, w, quantize_graph.quantize_weights(desc, w, ranges.astype(np.float32)), om

    @property
    def qm(self):
        return self.build()[2]

    def frames(self):
        """every frame the calls feed, in order"""
        return ic.all_frames([ic.Tracks(lengths, pads, seed=self.seed + ci) for ci, (lengths, pads) in enumerate(self.calls)])


def gpu_calls(T, rng):
    """five ambient tracks of 31 000 - 32 000 frames (more than 2 x 256 tiles: the tile loop of a workgroup runs more than
    once), then 40 short positives with pads and the lengths T - 1, 0, 3"""
    amb = [int(v) for v in rng.integers(31000, 32000, 5)]
    pos = [int(v) for v in rng.integers(60, 200, 40)] + [T - 1, 0, 3]
    return [(amb, [0] * len(amb)), (pos, [min(int(v), L) for v, L in zip(rng.integers(0, 20, len(pos)), pos)])]


# random topologies ec.random_inception_flags(i) that meet the input condition at T = 60 (tests/test_inception_q8_cpu.py
# evaluates it for every case listed here).  They cover two stem layers (2, 3, 4, 7, 9), dilation 2 (2), sub-spectral groups
# > 1 in the stem (1, 2, 4, 6, 7, 9) and in a block (2, 3, 4, 6, 12).
SWEEP = (1, 2, 3, 4, 6, 7, 9, 12)
SWEEP_T = 60


def sweep_calls(i):
    rng = np.random.default_rng(700 + i)
    return [([int(rng.integers(280, 400)), int(rng.integers(1, 40)), 0], [0, 1, 0]), ([int(rng.integers(60, 120)), 5], [0, 5])]


def negative_minima(ranges):
    """every op's output range given a negative minimum (-0.3 of its maximum).  A calibrated range of a ReLU output starts at
    0, which puts its zero point at -128, where the fused ReLU's clamp to max(-128, zp_out) cannot be told from the int8
    saturation; with these ranges the zero points are near -69 and every negative accumulator meets the clamp."""
    ranges[1:-1, 0] = -0.3 * ranges[1:-1, 1]
    return ranges


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for name, (flags, T) in ic.EMU_TOPOLOGIES.items():
        out["emu/" + name] = Case("emu/" + name, T, ic._emu_calls(T), flags=flags)
    for f1 in (10, 16):
        out["emu/FUSED_%d" % f1] = Case("emu/FUSED_%d" % f1, 60, ic._emu_calls(60), desc=fused_description(f1, 60))
    out["emu/RELU_ZP"] = Case("emu/RELU_ZP", 60, ic._emu_calls(60), flags=ec.INC, range_edit=negative_minima)
    out["emu/BIG"] = Case("emu/BIG", 60, ic._emu_calls(60), desc=big_description(60))
    out["emu/MID"] = Case("emu/MID", 60, ic._emu_calls(60), desc=big_description(60, 128))
    for name, (flags, T) in ic.GPU_TOPOLOGIES.items():
        out["gpu/" + name] = Case("gpu/" + name, T, gpu_calls(T, np.random.default_rng(1)), flags=flags)
    for i in SWEEP:
        out["sweep/%d" % i] = Case("sweep/%d" % i, SWEEP_T, sweep_calls(i), flags=ec.random_inception_flags(i), seed=50 + i)
    return out


# ------------------------------------------------------------------------------------------------- input condition

def spread(qm, frames):
    """(distinct int8 logits, share of the most frequent one, largest share of a ring-feeding tensor's values at a clamp
    value) of the ORACLE over ``frames`` from reset - what an int8 comparison on these inputs can see at all"""
    trace = []
    _, logit, _ = qgo.whole_sequence(qm, frames, trace=trace)
    vals, counts = np.unique(logit, return_counts=True)
    clamped = 0.0
    for relu, zp, a in trace:
        if a.size:
            lo = max(-128, zp) if relu else -128
            clamped = max(clamped, float(np.mean((a == lo) | (a == 127))))
    return int(vals.size), float(counts.max() / max(1, logit.size)), clamped


def check_spread(qm, frames, what=""):
    distinct, share, clamped = spread(qm, frames)
    assert distinct >= qc.SPREAD_MIN_DISTINCT and share <= qc.SPREAD_MAX_SHARE and clamped <= qc.SPREAD_MAX_CLAMPED, (
        what, "distinct logits %d, most frequent %.3f, clamped %.3f" % (distinct, share, clamped))
    return distinct, share, clamped


# -------------------------------------------------------------------------------------------------------- the kernel

def context_model(lib, case):
    """a float model whose context (device, HIP stream, stores) the int8 stream borrows; for a flag case the case's own"""
    if case.flags is not None:
        model = ic.make_model(lib, case.flags, case.T, case.model_seed)[1]
    else:
        model = ic.make_model(lib, ec.INC, case.T)[1]
    return model


def _check_probs(qsm, u8):
    p = qsm.read_probabilities()
    assert np.array_equal(p.view(np.uint32), (u8.astype(np.float32) * qgo.INV255).view(np.uint32))


def check_q8_stream_parity(lib, case, model=None, qm=None, calls=None):
    """the case's calls as successive mww_stream_run calls on one int8 graph stream: uint8 outputs, int8 logits, int8 rings
    after every call and the probabilities (bitwise u8 * float32(1/255)) equal the oracle's.  Returns (model, outputs)."""
    model = model or context_model(lib, case)
    qm = qm or case.qm
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    assert qsm.native.num_tensors() == len(qm.desc["conv_ops"]) + 2
    _, _, st0 = qgo.whole_sequence(qm, np.zeros((0, 40), np.float32))
    assert np.array_equal(qsm.get_state_q8(), st0), "rings at reset are not the zero points"
    done, outs = [], []
    for ci, (lengths, pads) in enumerate(calls or case.calls):
        tr = ic.Tracks(lengths, pads, seed=case.seed + ci).upload(model, (2 * ci, 2 * ci + 1))
        off = qsm.native.run(tr.win)
        u8 = qsm.read_q8()
        assert off[-1] == u8.size and list(np.diff(off)) == list(lengths)
        done.append(tr)
        ref_u8, ref_lq, ref_st = qgo.whole_sequence(qm, ic.all_frames(done))
        assert np.array_equal(u8, ref_u8[ref_u8.size - u8.size:]), "%s call %d: %d of %d outputs differ" % (
            case.name, ci, int(np.sum(u8 != ref_u8[ref_u8.size - u8.size:])), u8.size)
        qc.check_logits(qsm, ref_lq[ref_lq.size - u8.size:], "%s call %d" % (case.name, ci))
        assert np.array_equal(qsm.get_state_q8(), ref_st), "%s call %d: rings differ" % (case.name, ci)
        _check_probs(qsm, u8)
        outs.append(u8)
    return model, outs


def check_q8_non_stream(lib, case, lengths, pads, model=None, seed=0):
    model = model or context_model(lib, case)
    qsm = streaming.QuantizedStreamingModel(case.qm, 1, "non_stream", context=model)
    tr = ic.Tracks(lengths, pads, seed=seed).upload(model)
    off = qsm.native.run(tr.win)
    u8 = qsm.read_q8()
    lq = []
    for t, f in enumerate(tr.frames):
        ref_u8, ref_lq = qgo.non_stream(case.qm, f, case.T, want_logits=True)
        assert np.array_equal(u8[off[t]:off[t + 1]], ref_u8), "track %d" % t
        lq.append(ref_lq)
    qc.check_logits(qsm, np.concatenate(lq + [np.zeros(0, np.int8)]), "non_stream")
    _check_probs(qsm, u8)
    return qsm


def check_stream_equals_non_stream_past_warmup(lib, case, lengths, model=None, seed=5):
    """stream mode from reset, one track at a time, equals non_stream on every window: stream output T - 1 + i has the
    receptive field of window i (no ring is read past the first T - 1 outputs)"""
    model = model or context_model(lib, case)
    T = case.T
    a = streaming.QuantizedStreamingModel(case.qm, 1, "stream", context=model)
    b = streaming.QuantizedStreamingModel(case.qm, 1, "non_stream", context=model)
    tr = ic.Tracks(lengths, seed=seed).upload(model)
    for t in range(len(lengths)):
        a.reset()
        a.native.run(tr.win[t:t + 1])
        st = a.read_q8()
        b.native.run(tr.win[t:t + 1])
        ns = b.read_q8()
        assert ns.size == lengths[t] - T + 1 > 0
        assert np.array_equal(st[T - 1:], ns), "track %d" % t


def check_bit_identical(lib, case, lengths, model=None, seed=4):
    """two fresh int8 streams agree bit for bit; reset() restores the zero-point rings, after which the run repeats itself"""
    model = model or context_model(lib, case)
    tr = ic.Tracks(lengths, seed=seed).upload(model)
    out = []
    for _ in range(2):
        qsm = streaming.QuantizedStreamingModel(case.qm, 1, "stream", context=model)
        st0 = qsm.get_state_q8()
        qsm.native.run(tr.win)
        out.append((qsm.read_q8(), qsm.native.read(want_logits=True)[1], qsm.get_state_q8()))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert np.any(out[0][2] != st0)
    qsm.reset()
    assert np.array_equal(qsm.get_state_q8(), st0)
    qsm.native.run(tr.win)
    assert np.array_equal(qsm.read_q8(), out[0][0])


def check_calibration(lib, flags, T, n_frames, seed=11):
    """the recorded ranges of the float graph stream: the logit range is min / max of the float stream's own logits on the
    same frames bit for bit, the input range is that of the fed frames, every other range is within RANGE_RTOL (relative
    to the tensor's largest magnitude) of the float64 restatement, and recording leaves probabilities and state unchanged"""
    om, model = ic.make_model(lib, flags, T)
    frames = qc.calibration_set(n_frames, seed)
    desc = streaming.graph_stream_description(flags, T, 1, "stream")
    flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()])
    a = native.GraphStream(model.engine, desc, int8=True)
    a.set_weights(flat)
    ranges = a.calibrate_host(frames)
    assert ranges.shape == (len(desc["conv_ops"]) + 2, 2)
    p_cal = a.read()
    b = native.GraphStream(model.engine, desc)   # the plain creator: the float kernel as it runs in evaluation
    b.set_weights(flat)
    b.run_host(frames)
    p, z = b.read(want_logits=True)
    assert np.array_equal(p_cal.view(np.uint32), p.view(np.uint32))
    assert np.array_equal(a.get_state().view(np.uint32), b.get_state().view(np.uint32))
    assert ranges[-1, 0] == z.min() and ranges[-1, 1] == z.max()
    assert ranges[0, 0] == frames.min() and ranges[0, 1] == frames.max()
    ref = float64_ranges(om, flags, frames)
    assert ranges.shape == ref.shape
    for t, (got, want) in enumerate(zip(ranges.astype(np.float64), ref)):
        mag = max(abs(want[0]), abs(want[1]), 1e-30)
        assert np.all(np.abs(got - want) <= RANGE_RTOL * mag), (t, got, want)
    return model, ranges
