"""Checks of the int8 streaming evaluation (csrc/tu_stream_q8.hip through microwakeword_amd.quantize / streaming) shared by
the emulator tests (tests/test_stream_q8_emulated.py, small sizes) and the GPU tests (tests/test_stream_q8_gpu.py).  The
kernel is held bit for bit to tests/quant_oracle.py; the calibration to the float stream and the float64 oracle."""
import numpy as np

from microwakeword_amd import quantize, streaming
import quant_oracle as qo
import streaming_checks as sc
import streaming_oracle as so

RANGE_RTOL = 1e-5


def calibration_set(n_frames, seed=11):
    """frames shaped like the features: u16-scaled values, one pixel at 0 and one at 26 (the calibration's fixed pixels)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 900, size=(n_frames, 40)).astype(np.float32) * np.float32(0.0390625)
    x[0, 0], x[0, 1] = 0.0, 26.0
    return x


def make_quantized(lib, flags, T, cal_frames=400, seed=42):
    """(oracle model, float Model, QuantizedModel) calibrated on a synthetic calibration stream"""
    om, model = sc.make_model(lib, flags, T, seed=seed)
    sm = streaming.StreamingModel(model, int(flags["stride"]), "stream")
    ranges = sm.native.calibrate_host(calibration_set(cal_frames))
    sm.native.close()
    return om, model, quantize.quantize(model, ranges)


def synthetic_quantized(desc, seed=0, ranges=None):
    """a QuantizedModel of any stream description from random Keras-order weights and fixed ranges (topologies no float
    engine instantiates, e.g. tiles too large for LDS); run it with the context of any float model.  ``ranges``
    [n_tensors, 2] replaces the fixed ranges (which leave odd topologies with a near-constant logit: see check_spread)."""
    fixed = ranges is None
    rng = np.random.default_rng(seed)
    k1, c = int(desc["conv1_kernel"]), int(desc["conv1_filters"])
    w = [rng.normal(0, 0.1, (k1, 1, 40, c))]
    fixed_ranges, ranges = ranges, [(0.0, 26.0), (0.0, 4.0)]
    for kind, _, _, ks, ci, co in quantize.plan_ops(desc):
        if kind == "mix":
            for gc, k in zip(quantize.split_channels(ci, len(ks)), ks):
                w += [rng.normal(0, 0.3, (k, 1, gc, 1)), rng.normal(0, 0.1, gc)]
            ranges.append((-4.0, 4.0))
        else:
            w += [rng.normal(0, 0.2, (1, 1, ci, co)), 1 + rng.random(co), rng.normal(0, 0.1, co), rng.normal(0, 0.1, co),
                  1 + rng.random(co)]
            ranges.append((0.0, 4.0))
    c_last = int(desc["blocks"][-1][2])
    w += [rng.normal(0, 0.05, (int(desc["t_final"]) * c_last, 1)), rng.normal(0, 0.1, 1)]
    ranges.append((-8.0, 8.0))
    if not fixed:
        ranges = fixed_ranges
    return quantize.quantize_weights(desc, w, np.array(ranges, np.float32))


SPREAD_MIN_DISTINCT, SPREAD_MAX_SHARE, SPREAD_MAX_CLAMPED = 32, 0.5, 0.9


def spread(qm, frames):
    """(distinct int8 logits, share of the most frequent one, largest share of a ring-feeding tensor's values at a clamp
    value) of the ORACLE over ``frames`` from reset - what an int8 comparison on these inputs can see at all"""
    trace = []
    _, logit, _ = qo.whole_sequence(qm, frames, trace=trace)
    vals, counts = np.unique(logit, return_counts=True)
    clamped = 0.0
    for relu, zp, a in trace:
        if a.size:
            lo = max(-128, zp) if relu else -128
            clamped = max(clamped, float(np.mean((a == lo) | (a == 127))))
    return int(vals.size), float(counts.max() / max(1, logit.size)), clamped


def check_spread(qm, frames, what=""):
    """a condition on the INPUTS of an int8 comparison, from the oracle alone: at least 32 distinct logits, none more
    than half of the time, no ring-feeding tensor more than 90 % at its clamp values"""
    distinct, share, clamped = spread(qm, frames)
    assert distinct >= SPREAD_MIN_DISTINCT and share <= SPREAD_MAX_SHARE and clamped <= SPREAD_MAX_CLAMPED, (
        what, "distinct logits %d, most frequent %.3f, clamped %.3f" % (distinct, share, clamped))
    return distinct, share, clamped


def check_logits(qsm, ref_lq, what):
    """the kernel's int8 logit (float32 in the logit buffer) equals the oracle's: the uint8 output is a many-to-one table
    of it (a handful of distinct outputs from tens of logits), so this is where a Dense / requantization error shows"""
    lq = qsm.native.read(want_logits=True)[1]
    ref = np.asarray(ref_lq, np.float32)
    assert lq.shape == ref.shape, (what, lq.shape, ref.shape)
    assert np.array_equal(lq, ref), "%s: %d of %d int8 logits differ (largest difference %g)" % (
        what, int(np.sum(lq != ref)), lq.size, float(np.abs(lq - ref).max()))


def _check_probs(qsm, u8):
    p = qsm.read_probabilities()
    assert np.array_equal(p.view(np.uint32), (u8.astype(np.float32) * qo.INV255).view(np.uint32))


def check_q8_stream_parity(lib, flags, T, calls, seed=0, qm=None, model=None):
    """``calls``: (lengths, pads) run as successive mww_stream_run calls on one int8 stream; uint8 outputs, int8 logits
    and int8 rings after every call equal the oracle's.  Returns (model, qm, per-call uint8 outputs)."""
    if qm is None:
        _, model, qm = make_quantized(lib, flags, T)
    s = int(flags["stride"])
    qsm = streaming.QuantizedStreamingModel(qm, s, "stream", context=model)
    fed, outs = [], []
    for ci, (lengths, pads) in enumerate(calls):
        tr = sc.Tracks(model, lengths, pads, seed=seed + ci, store_ids=(2 * ci, 2 * ci + 1))
        off = qsm.native.run(tr.win)
        u8 = qsm.read_q8()
        assert off[-1] == u8.size
        for t in range(len(lengths)):
            assert off[t + 1] - off[t] == lengths[t] // s
        fed += [f[:(len(f) // s) * s] for f in tr.frames]
        ref_u8, ref_lq, ref_st = qo.whole_sequence(qm, np.concatenate(fed + [np.zeros((0, 40), np.float32)], 0))
        assert np.array_equal(u8, ref_u8[ref_u8.size - u8.size:]), "call %d: %d of %d outputs differ" % (
            ci, int(np.sum(u8 != ref_u8[ref_u8.size - u8.size:])), u8.size)
        check_logits(qsm, ref_lq[ref_lq.size - u8.size:], "call %d" % ci)
        assert np.array_equal(qsm.get_state_q8(), ref_st), "call %d: rings differ" % ci
        _check_probs(qsm, u8)
        outs.append(u8)
    return model, qm, outs


def check_q8_non_stream(lib, flags, T, lengths, pads, seed=0, qm=None, model=None):
    if qm is None:
        _, model, qm = make_quantized(lib, flags, T)
    qsm = streaming.QuantizedStreamingModel(qm, int(flags["stride"]), "non_stream", context=model)
    tr = sc.Tracks(model, lengths, pads, seed=seed)
    off = qsm.native.run(tr.win)
    u8 = qsm.read_q8()
    lq = []
    for t, f in enumerate(tr.frames):
        ref_u8, ref_lq = qo.non_stream(qm, f, T, want_logits=True)
        assert np.array_equal(u8[off[t]:off[t + 1]], ref_u8), "track %d" % t
        lq.append(ref_lq)
    check_logits(qsm, np.concatenate(lq + [np.zeros(0, np.int8)]), "non_stream")
    _check_probs(qsm, u8)
    return qsm, tr, off, u8


def check_stream_equals_non_stream_past_warmup(model, qm, flags, T, lengths, seed=5):
    """stream mode from reset, one track at a time, equals non_stream on every window past the receptive field"""
    s = int(flags["stride"])
    a = streaming.QuantizedStreamingModel(qm, s, "stream", context=model)
    b = streaming.QuantizedStreamingModel(qm, s, "non_stream", context=model)
    tr = sc.Tracks(model, lengths, seed=seed)
    o = T % s   # stream output j ends at frame (j + 1) * s: start the stream o frames in so that it meets the windows' ends
    for t in range(len(lengths)):
        a.reset()
        w = tr.win[t:t + 1].copy()
        w["src_elem"] += o * 40
        w["copy_rows"] -= o
        a.native.run(w)
        st = a.read_q8()
        b.native.run(tr.win[t:t + 1])
        ns = b.read_q8()
        # non_stream window i = frames [i * s, i * s + T) ends at o + (T // s + i) * s: stream output T // s - 1 + i, whose
        # receptive field is that window; past the warm-up (no ring read) once i * s >= o
        j0, i0 = T // s - 1, (1 if o else 0)
        assert ns.size == max(0, (lengths[t] - T) // s + 1)
        assert ns.size > i0
        assert np.array_equal(st[j0 + i0:j0 + ns.size], ns[i0:]), "track %d" % t


def float64_ranges(om, flags, frames):
    """[min, max] of every tensor of the float64 streaming oracle over the fed frames from zero state"""
    net = so.Net(flags, om)
    s = net.s
    F = (len(frames) // s) * s
    n = F // s
    x64 = np.asarray(frames[:F], np.float64)
    out = [(x64.min(), x64.max())]
    a = net.conv1(np.concatenate([np.zeros((net.r1, 40)), x64], 0))[:n]
    out.append((a.min(), a.max()))
    for kind, p, ks in net.layers:
        if kind == "mix":
            a = net.mix(p, ks, np.concatenate([np.zeros((max(ks) - 1, a.shape[1])), a], 0))
        else:
            a = net.pw(p, a)
        out.append((a.min(), a.max()))
    z = so.whole_sequence(net, x64)
    out.append((z.min(), z.max()))
    return np.array(out, np.float64)


def check_calibration(lib, flags, T, n_frames, seed=11):
    """the recorded ranges: the logit range is min / max of the float stream's own logits on the same frames bit for bit,
    the input range is that of the fed frames, every range is within RANGE_RTOL (relative to the tensor's largest
    magnitude) of the float64 oracle, and recording leaves the probabilities unchanged"""
    om, model = sc.make_model(lib, flags, T)
    s = int(flags["stride"])
    frames = calibration_set(n_frames, seed)
    a = streaming.StreamingModel(model, s, "stream")
    ranges = a.native.calibrate_host(frames)
    p_cal = a.native.read()
    b = streaming.StreamingModel(model, s, "stream")
    b.native.run_host(frames)
    p, z = b.native.read(want_logits=True)
    assert np.array_equal(p_cal.view(np.uint32), p.view(np.uint32))
    assert np.array_equal(a.native.get_state(), b.native.get_state())
    assert ranges[-1, 0] == z.min() and ranges[-1, 1] == z.max()
    fed = frames[:(n_frames // s) * s]
    assert ranges[0, 0] == fed.min() and ranges[0, 1] == fed.max()
    ref = float64_ranges(om, flags, frames)
    assert ranges.shape == ref.shape
    for t, (got, want) in enumerate(zip(ranges.astype(np.float64), ref)):
        mag = max(abs(want[0]), abs(want[1]), 1e-30)
        assert np.all(np.abs(got - want) <= RANGE_RTOL * mag), (t, got, want)
    return ranges
