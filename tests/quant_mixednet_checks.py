"""Checks of the int8 streaming evaluation of MixedNets with residual connections or a pooled head
(``mww_stream_create_mixednet_q8``, stream_q8_kernel<true> of csrc/tu_stream_q8.hip through microwakeword_amd.quantize_mixednet / streaming)
shared by the emulator tests (tests/test_mixednet_q8_emulated.py) and the GPU tests (tests/test_mixednet_q8_gpu.py).

- ``case_ids()``: every non-attention case of ``mixednet_variant_checks.cases()`` (imported, not edited: their stream scripts
  and their non_stream twins) plus four of this file: ``wide-scratch`` (a tile above 160 KB: the global-scratch form),
  ``default48`` (the default widths with residual 1,0,1,0 and average pooling: the three-buffer tile above 64 KB of LDS),
  ``relu-clamp`` (hand-set negative range minima, so that the ADD's fused-ReLU clamp is not the int8 floor) and ``add-rounding``
  (hand-set ADD scales in the ratio 7 : 1.5 : 1, where the rounding of the ADD's scaled inputs decides exact ties of the output).
- ``oracle_model(cid)``: the int8 model of a case WITHOUT a device - the ranges of the float64 streaming oracle over the
  calibration frames - on which the CPU test asserts the input conditions (``conditions``).
- ``run_case(lib, cid, n_cu)``: the model calibrated ON THE DEVICE (400 synthetic frames; hand-set ranges for ``relu-clamp`` and ``add-rounding``),
  the calibration held to the old creator's run and to the float64 oracle, then every call of the script, the chunked runs and
  the non_stream twin bit for bit against tests/quant_mixednet_oracle.py: uint8 outputs, int8 logits, int8 rings, probabilities.
"""
import functools
import time

import numpy as np

import engine_checks as ec
import mixednet_variant_checks as vc
import mixednet_variant_streaming_oracle as vo
import q8_checks as qc
import quant_mixednet_oracle as qmo
import stream_sweep as sw
import streaming_checks as sc
from microwakeword_amd import native, quantize_mixednet as qmx

CAL_FRAMES = 400
ENVELOPE_PERIOD = 600   # frames
TILE = sw.TILE
DEFAULT48 = vc.desc_of(32, 5, 3, [(1, (5,), 48), (1, (9,), 48), (1, (13,), 48), (1, (21,), 48)], 3, residual=[1, 0, 1, 0], pool="average")


def _extra_cases():
    return [
        # the tile - gathered rows and three int8 buffers of 259 rows x 208 channels - exceeds 160 KB: per-workgroup global scratch
        vc.Case("wide-scratch", vc.desc_of(8, 3, 1, [(1, (3,), 208)], 2, residual=[1]),
                script=[("tracks", [300, 0, 40], [0, 0, 3]), ("host", 270), ("reset",), ("outputs", 257)], ns=([8, 5, 270], [2, 0, 0]), cap=280),
        # the default widths: the only case whose three-buffer tile lies between 64 KB and 160 KB of LDS
        vc.Case("default48", DEFAULT48, script=[("tracks", [400, 0, 350, 7], [0, 0, 5, 0]), ("zero",), ("host", 300), ("reset",), ("ones", 3),
                                                ("tracks", [260 * 3 + 1], [0])], cap=300),
        # as the first case of mixednet_variant_checks, with hand-set ranges (``hand_ranges``)
        vc.Case("relu-clamp", vc.desc_of(6, 5, 2, [(2, (3,), 8), (1, (3, 5), 8), (1, (3,), 5)], 3, residual=[1, 0, 1]),
                script=[("tracks", [0, 7, 90, 0, 3, 61, 0], [0, 2, 0, 0, 0, 4, 0]), ("host", 50), ("reset",), ("ones", 4)], cap=300),
        # two repeats of one residual block whose ADD scales are hand-set (``ADD_ROUNDING_WIDTHS``)
        vc.Case("add-rounding", vc.desc_of(6, 3, 1, [(2, (3,), 8)], 3, residual=[1]),
                script=[("tracks", [120, 0, 33], [0, 0, 4]), ("host", 70), ("reset",), ("ones", 3)], cap=300),
    ]


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [c for c in vc.cases() if not c.desc["attention"]] + _extra_cases()
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


def case_ids():
    return [c.id for c in _cases()]


def case(cid):
    return next(c for c in _cases() if c.id == cid)


def gen_frames(rng, n, kind="f32", phase=0):
    """``stream_sweep.gen_frames`` under a slow envelope (0.2 .. 1 of the amplitude, period ENVELOPE_PERIOD frames, ``phase``:
    frames fed before these): identically distributed frames leave a head that averages 300 of them with ONE int8 logit once
    it is warm, which an int8 comparison cannot tell from a constant"""
    env = 0.2 + 0.4 * (1 + np.sin(2 * np.pi * (np.arange(n) + phase) / ENVELOPE_PERIOD))
    return (sw.gen_frames(rng, n, kind) * env[:, None].astype(np.float32)).astype(np.float32)


def calibration_frames(cid):
    """400 synthetic calibration frames of the distribution the case's calls feed, with the calibration's two fixed pixels"""
    x = gen_frames(sw._rng(cid, 2), CAL_FRAMES, "u16")
    x[0, 0], x[0, 1] = 0.0, 26.0
    return x


@functools.lru_cache(maxsize=None)
def seq_of(cid):
    """the case's long sequence (the chunked runs, the input conditions): cap x stride frames"""
    c = case(cid)
    return gen_frames(sw._rng(cid, 1), c.cap * c.desc["stride"], "u16")


def tile_bytes(desc):
    """bytes of one int8 tile (MixedNet::plan restated): the gathered input rows and (2 + has_res) activation buffers"""
    rows = TILE + sw.reach1_of(desc)
    return ((rows - 1) * desc["stride"] + desc["conv1_kernel"]) * 40 + (2 + int(any(desc["residual"]))) * rows * sw.r4(sw.cmax_of(desc))


@functools.lru_cache(maxsize=None)
def built(cid):
    """as mixednet_variant_checks.built, for the cases of this file too"""
    if cid in vc.case_ids():
        return vc.built(cid)
    c = case(cid)
    b = vc.Built()
    b.case, b.desc = c, c.desc
    b.flags = vc.flags_of(c.desc)
    b.T, b.s = c.desc["frames"], c.desc["stride"]
    om = ec.perturbed_oracle(b.T, seed=vc.SEED, flags=b.flags)
    assert vo.t_final_of(b.flags, b.T) == c.desc["t_final"], cid
    b.seq = sw.gen_frames(sw._rng(cid, 0), c.cap * b.s, "u16")
    b.om = vc._condition_bn(b.flags, om, b.T, b.seq, c.bn_shift)
    b.net = vo.Net(b.flags, b.om, b.T)
    b.weights = b.om.get_weights()
    b.flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in b.weights])
    return b


def desc_of(b):
    """the description the quantized model carries: the head options dropped when T_f = 1"""
    return qmx.normalized(b.desc)


# ------------------------------------------------------------------------------------------------ float64 ranges
def float64_ranges(b, frames):
    """[min, max] of every tensor (``quantize_mixednet.tensor_names``) of the float64 streaming oracle over the fed frames from
    zero state; a residual block's 1x1 is recorded before the add and after add + ReLU"""
    net = b.net
    s = net.s
    F = (len(frames) // s) * s
    x64 = np.asarray(frames[:F], np.float64)
    out = [(x64.min(), x64.max())]
    a = net.conv1(np.concatenate([np.zeros((net.r1, 40)), x64], 0))[:F // s]
    out.append((a.min(), a.max()))
    r = {}
    for kind, p, ks in net.layers:
        if kind == "res":
            r[p] = net.res(p, a)
            out.append((r[p].min(), r[p].max()))
        elif kind == "mix":
            a = net.mix(p, ks, np.concatenate([np.zeros((max(ks) - 1, a.shape[1])), a], 0))
            out.append((a.min(), a.max()))
        elif ks:
            y = net._bn(a @ net.w[p + ".pw.kernel"][0, 0], p + ".bn")
            a = np.maximum(y + r[ks], 0)
            out += [(y.min(), y.max()), (a.min(), a.max())]
        else:
            a = net.pw_res(p, a, None)
            out.append((a.min(), a.max()))
    z = vo.whole_sequence(net, x64)
    out.append((z.min(), z.max()))
    return np.array(out, np.float64)


def hand_ranges(ranges, names):
    """``relu-clamp``: every tensor behind a ReLU (conv1, a plain 1x1, an ADD) gets a negative range minimum of a third of its
    maximum, so its zero point lies above -128 and the fused clamp cuts values the int8 floor would keep"""
    out = np.array(ranges, np.float64)
    for t, n in enumerate(names):
        if n == "conv1" or n.endswith(".add") or (n.endswith(".pointwise") and n[:-len("pointwise")] + "add" not in names):
            out[t, 0] = -out[t, 1] / 3
    return out


# ``add-rounding``: range widths 255 x scale with the scales 7/64 (the 1x1 output), 1.5/64 (r) and 1/64 (the ADD output), all
# exact in float32.  The 1x1 input contributes 7 d1 to the output exactly (multiplier 1/2, no shift; output multiplier 14 / 2^20,
# mantissa 0.875, exact).  r contributes 1.5 d2 - an exact tie for every odd d2, which the contract rounds away from zero - through
# the multiplier 1.5 / 14 and a right shift.  Without RoundingDivideByPOT's rounding term the scaled r is the floor, up to one
# unit below; 0.875 of that unit, rounded by the output stage's SaturatingRoundingDoublingHighMul, puts the sum one below the
# tie whenever the dropped fraction exceeds 4/7, and the output comes out one smaller.
ADD_ROUNDING_WIDTHS = {"pointwise": 255 * 7 / 64, "residual": 255 * 1.5 / 64, "add": 255 / 64}


def add_rounding_ranges(ranges, names):
    out = np.array(ranges, np.float64)
    for t, n in enumerate(names):
        kind = n.rsplit(".", 1)[-1]
        if n.startswith("block0.") and kind in ADD_ROUNDING_WIDTHS:
            w = ADD_ROUNDING_WIDTHS[kind]
            out[t] = (-w / 4, 3 * w / 4) if kind == "add" else (-w / 2, w / 2)
    return out


def _final_ranges(cid, ranges):
    names = qmx.tensor_names(desc_of(built(cid)))
    if cid == "relu-clamp":
        return hand_ranges(ranges, names)
    return add_rounding_ranges(ranges, names) if cid == "add-rounding" else ranges


@functools.lru_cache(maxsize=None)
def oracle_model(cid):
    """the int8 model from the float64 oracle's ranges over the calibration frames: no device"""
    b = built(cid)
    return qmx.quantize_weights(desc_of(b), b.weights, _final_ranges(cid, float64_ranges(b, calibration_frames(cid))))


# ---------------------------------------------------------------------------------------------- input conditions
ADD_MIN_DISTINCT = 16


def conditions(qm, frames, what=""):
    """Conditions on the INPUTS of an int8 comparison, from the oracle alone.  The three of ``q8_checks.check_spread`` - at
    least 32 distinct int8 logits, none of them more than half of the time, no ring-feeding tensor more than 90 % at a clamp
    value -; per ADD: its output not more than 90 % at a clamp value and both operands with at least 16 distinct values.
    Returns dict(distinct, share, clamped, adds=[(distinct 1x1, distinct r, clamped share)], pool_acc=[accumulators])."""
    trace, adds, pools = [], [], []
    _, logit, _ = qmo.whole_sequence(qm, frames, trace=trace, add_trace=adds, pool_trace=pools)
    vals, counts = np.unique(logit, return_counts=True)
    clamped = 0.0
    for relu, zp, a in trace:
        if a.size:
            lo = max(-128, zp) if relu else -128
            clamped = max(clamped, float(np.mean((a == lo) | (a == 127))))
    distinct, share = int(vals.size), float(counts.max() / max(1, logit.size))
    assert distinct >= qc.SPREAD_MIN_DISTINCT and share <= qc.SPREAD_MAX_SHARE and clamped <= qc.SPREAD_MAX_CLAMPED, (
        what, "distinct logits %d, most frequent %.3f, clamped %.3f" % (distinct, share, clamped))
    add_figs = []
    for q1, r, out, zo, _, _, _ in adds:
        fig = (int(np.unique(q1).size), int(np.unique(r).size), float(np.mean((out == max(-128, zo)) | (out == 127))))
        assert fig[0] >= ADD_MIN_DISTINCT and fig[1] >= ADD_MIN_DISTINCT and fig[2] <= qc.SPREAD_MAX_CLAMPED, (what, "ADD", fig)
        add_figs.append(fig)
    return dict(distinct=distinct, share=share, clamped=clamped, adds=add_figs, pool_acc=pools)


# ------------------------------------------------------------------------------------------------------- device
def new_float_stream(lib, b, int8, mode="stream"):
    st = native.Stream(sc.context_model(lib).engine, dict(b.desc, mode=mode), int8=int8)
    st.set_weights(b.flat)
    return st


def new_q8_stream(lib, qm, mode="stream"):
    st = native.Stream(sc.context_model(lib).engine, dict(qm.desc, mode=mode), int8=True)
    st.set_quantized(*qm.packed())
    return st


def check_calibration(lib, cid):
    """``calibrate_host`` on a stream of the new creator: probabilities and rings equal ``run_host`` on a stream of the OLD
    creator bit for bit, the ranges equal the float64 oracle's within ``q8_checks.RANGE_RTOL`` of each tensor's largest
    magnitude, the logit range is that of the run's own logits.  Returns the ranges."""
    b = built(cid)
    frames = calibration_frames(cid)
    a = new_float_stream(lib, b, True)
    assert a.num_tensors() == len(qmx.tensor_names(desc_of(b))), cid
    ranges = a.calibrate_host(frames)
    p_cal, st_cal = a.read(), a.get_state()
    a.close()
    o = new_float_stream(lib, b, False)
    o.run_host(frames)
    p, z = o.read(want_logits=True)
    assert np.array_equal(p_cal.view(np.uint32), p.view(np.uint32)), cid + ": recording changed the probabilities"
    assert np.array_equal(st_cal.view(np.uint32), o.get_state().view(np.uint32)), cid + ": recording changed the rings"
    o.close()
    assert ranges[-1, 0] == z.min() and ranges[-1, 1] == z.max()
    fed = frames[:(len(frames) // b.s) * b.s]
    assert ranges[0, 0] == fed.min() and ranges[0, 1] == fed.max()
    ref = float64_ranges(b, frames)
    assert ranges.shape == ref.shape, (cid, ranges.shape, ref.shape)
    for t, (got, want) in enumerate(zip(ranges.astype(np.float64), ref)):
        mag = max(abs(want[0]), abs(want[1]), 1e-30)
        assert np.all(np.abs(got - want) <= qc.RANGE_RTOL * mag), (cid, t, got, want)
    return ranges


class _Session:
    """one int8 stream of a case driven through the script, every call held to the oracle bit for bit"""

    def __init__(self, lib, b, qm, n_cu):
        self.b, self.qm, self.n_cu = b, qm, n_cu
        self.model = sc.context_model(lib)
        self.st = new_q8_stream(lib, qm)
        self._reset_oracle()

    def _reset_oracle(self):
        self.fed, self.n_fed, self.only_ones = [], 0, True
        self.step = qmo.StepStreamQ8(self.qm)

    def _check(self, n_new, what, step_ref=None):
        u8 = self.st.read_q8()
        p, z = self.st.read(want_logits=True)
        assert u8.size == n_new, (what, u8.size, n_new)
        if step_ref is not None:
            ref_lq, ref_st = step_ref
            ref_u8 = self.step.q.output(ref_lq)[0]
        else:
            ref_u8, ref_lq, ref_st = qmo.whole_sequence(self.qm, np.concatenate(self.fed + [np.zeros((0, 40), np.float32)], 0))
            ref_u8, ref_lq = ref_u8[ref_u8.size - n_new:], ref_lq[ref_lq.size - n_new:]
        assert np.array_equal(u8, ref_u8), "%s: %d of %d outputs differ" % (what, int(np.sum(u8 != ref_u8)), n_new)
        assert np.array_equal(z, np.asarray(ref_lq, np.float32)), "%s: %d of %d int8 logits differ" % (
            what, int(np.sum(z != np.asarray(ref_lq, np.float32))), n_new)
        assert np.array_equal(p.view(np.uint32), (u8.astype(np.float32) * qmo.INV255).view(np.uint32)), what + ": probabilities"
        got_st = self.st.get_state_q8()
        assert np.array_equal(got_st, ref_st), "%s: %d of %d ring bytes differ" % (what, int(np.sum(got_st != ref_st)), ref_st.size)

    def run(self, i):
        b, s = self.b, self.b.s
        st = b.case.script[i]
        what = "%s step %d %s" % (b.case.id, i, st[0])
        rng = sw._rng(b.case.id, 0, i)
        if st[0] == "reset":
            self.st.reset()
            self._reset_oracle()
        elif st[0] == "zero":
            before = self.st.get_state_q8()
            n = self.st.run_host(gen_frames(rng, s - 1))
            assert n == 0 and self.st.n_out == 0, what
            assert np.array_equal(before, self.st.get_state_q8()), what + ": a call without outputs changed the state"
        elif st[0] == "tracks":
            tr = sc.Tracks(self.model, st[1], st[2], seed=int(rng.integers(1 << 30)))
            off = self.st.run(tr.win)
            for t, L in enumerate(st[1]):
                assert off[t + 1] - off[t] == L // s, what
            self.fed += [f[:(len(f) // s) * s] for f in tr.frames]
            self.n_fed += sum((len(f) // s) * s for f in tr.frames)
            self.only_ones = False
            self._check(int(off[-1]), what)
        elif st[0] in ("host", "outputs"):
            L = st[1] if st[0] == "host" else ((2 * self.n_cu + 2) * TILE + 5 if st[1] == "grid" else st[1]) * s + (s - 1)
            x = gen_frames(rng, L, "u16" if i % 2 else "f32", self.n_fed)
            n = self.st.run_host(x)
            assert n == L // s, what
            self.fed.append(x[:(L // s) * s])
            self.n_fed += (L // s) * s
            self.only_ones = False
            self._check(n, what)
        elif st[0] == "ones":
            for j in range(st[1]):
                x = gen_frames(rng, s, "f32", self.n_fed)
                assert self.st.run_host(x) == 1, what
                self.fed.append(x)
                self.n_fed += s
                ref = None
                if self.only_ones:   # the literal ring form, one step per chunk
                    ref = (np.array([self.step.step(x)], np.int64).astype(np.int8), self.step.state())
                self._check(1, "%s call %d" % (what, j), ref)
        else:
            raise ValueError(st)


def _one_call(lib, qm, seq):
    st = new_q8_stream(lib, qm)
    st.run_host(seq)
    out = (st.read_q8(), st.read(), st.get_state_q8())
    st.close()
    return out


def _chunking(lib, b, qm):
    """two runs of one call are identical; a call split into pieces gives the same outputs and the same final state"""
    seq = seq_of(b.case.id)
    n_out = len(seq) // b.s
    u0, p0, s0 = _one_call(lib, qm, seq)
    assert u0.size == n_out
    ref_u8, _, ref_st = qmo.whole_sequence(qm, seq)
    assert np.array_equal(u0, ref_u8) and np.array_equal(s0, ref_st), b.case.id + ": the whole sequence"
    u1, p1, s1 = _one_call(lib, qm, seq)
    assert np.array_equal(u0, u1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32)) and np.array_equal(s0, s1), b.case.id + ": reruns differ"
    for si, pieces in enumerate(sw._splits(sw._rng(b.case.id, 77), n_out, b.s)):
        st = new_q8_stream(lib, qm)
        us = []
        for lo, hi in pieces:
            assert st.run_host(seq[lo:hi]) == (hi - lo) // b.s
            us.append(st.read_q8())
        assert np.array_equal(np.concatenate(us), u0), "%s split %d %s: outputs differ" % (b.case.id, si, pieces)
        assert np.array_equal(st.get_state_q8(), s0), "%s split %d %s: final state differs" % (b.case.id, si, pieces)
        st.close()


def _non_stream(lib, b, qm):
    """the non_stream twin against the oracle's non-streaming form on every window; a second run bit for bit"""
    model = sc.context_model(lib)
    lens, pads = b.case.ns
    tr = sc.Tracks(model, lens, pads, seed=vc.SEED)
    runs = []
    for _ in range(2):
        st = new_q8_stream(lib, qm, "non_stream")
        off = st.run(tr.win)
        runs.append((st.read_q8(), st.read(want_logits=True)))
        st.close()
    u8, (p, z) = runs[0]
    assert np.array_equal(u8, runs[1][0]) and np.array_equal(p.view(np.uint32), runs[1][1][0].view(np.uint32)), b.case.id + ": non_stream reruns differ"
    for t, f in enumerate(tr.frames):
        ref_u8, ref_lq = qmo.non_stream(qm, f, b.T, want_logits=True)
        assert np.array_equal(u8[off[t]:off[t + 1]], ref_u8), "%s non_stream track %d" % (b.case.id, t)
        assert np.array_equal(z[off[t]:off[t + 1]], ref_lq.astype(np.float32)), "%s non_stream track %d logits" % (b.case.id, t)
    assert np.array_equal(p.view(np.uint32), (u8.astype(np.float32) * qmo.INV255).view(np.uint32))


def run_case(lib, cid, n_cu=256):
    b = built(cid)
    t0 = time.time()
    ranges = check_calibration(lib, cid)
    qm = qmx.quantize_weights(desc_of(b), b.weights, _final_ranges(cid, ranges))
    fig = conditions(qm, seq_of(cid), cid)   # the calibrated model meets the input conditions too
    ses = _Session(lib, b, qm, n_cu)
    for i in range(len(b.case.script)):
        ses.run(i)
    ses.st.close()
    _chunking(lib, b, qm)
    _non_stream(lib, b, qm)
    return dict(id=cid, seconds=round(time.time() - t0, 2), tile_bytes=tile_bytes(b.desc), distinct_logits=fig["distinct"],
                share=round(fig["share"], 3), clamped=round(fig["clamped"], 3), adds=fig["adds"])


# --------------------------------------------------------------------------------------------------------- ABI
def check_abi(lib):
    """the new creator refuses attention in both modes, naming it; num_tensors = len(tensor_names); set_quantized with wrong
    sizes is refused; a description with no option set is the plain plan"""
    import pytest
    model = sc.context_model(lib)
    att = vc.desc_of(6, 3, 1, [(1, (3,), 8)], 5, attention=1)
    for mode in ("stream", "non_stream"):
        with pytest.raises(native.NativeError, match="error -3.*spatial_attention"):
            native.Stream(model.engine, dict(att, mode=mode), int8=True)
    for cid in ("res-first-last_cin-ne-f_rep2_s2-k1gt_tf3", "res-consecutive_cin-eq-f_rep3_nodw_g2_s1-k1eq_avg-tf2", "pooled-flags_tf1_plain"):
        b = built(cid)
        st = native.Stream(model.engine, b.desc, int8=True)
        names = qmx.tensor_names(desc_of(b))
        assert st.num_tensors() == len(names), (cid, st.num_tensors(), names)
        wq, iv, s0, lut = oracle_model(cid).packed()
        assert st.q8_sizes() == (wq.size, iv.size), (cid, st.q8_sizes(), wq.size, iv.size)
        for w2, i2 in ((wq[:-4], iv), (wq, iv[:-1]), (np.concatenate([wq, wq[:4]]), iv)):
            with pytest.raises(native.NativeError, match="error -1.*expected"):
                st.set_quantized(w2, i2, s0, lut)
        bad = iv.copy()
        bad[-1] = 300
        with pytest.raises(native.NativeError, match="zero points"):
            st.set_quantized(wq, bad, s0, lut)
        st.set_quantized(wq, iv, s0, lut)
        st.close()
    b = built("res-first-last_cin-ne-f_rep2_s2-k1gt_tf3")
    qm = oracle_model(b.case.id)
    wq, iv, s0, lut = qm.packed()
    at = sum(3 * op["bias"].size for op in qm.ops[:next(i for i, op in enumerate(qm.ops) if op["kind"] == "pw_add") + 1])
    bad = iv.copy()
    bad[at + 1] = 1   # sh1 > 0: not a multiplier below one
    st = native.Stream(model.engine, b.desc, int8=True)
    with pytest.raises(native.NativeError, match="ADD multipliers"):
        st.set_quantized(wq, bad, s0, lut)
    st.close()
    plain = {k: v for k, v in built("pooled-flags_tf1_plain").desc.items() if k not in ("residual", "attention", "pool")}
    a, c = native.Stream(model.engine, plain), native.Stream(model.engine, plain, int8=True)
    assert (a.n_weights, a.n_state, a.num_tensors(), a.q8_sizes()) == (c.n_weights, c.n_state, c.num_tensors(), c.q8_sizes())
    a.close()
    c.close()
