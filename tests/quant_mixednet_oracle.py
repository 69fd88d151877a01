"""TEST INFRASTRUCTURE: NumPy int64 restatement of the int8 streaming MixedNet with residual connections and a pooled head
(the contract in INTEGRATION.md 6, "residual and pooled MixedNets") from the parameters of a
``microwakeword_amd.quantize_mixednet.QuantizedMixedNetModel``, written apart from the kernel and from the package's packing
code: zero points are subtracted (the kernel folds them into the bias), the ADD's three multipliers are derived here from the
tensor scales, the ADD and the average-pool rounding are written from the contract's formulas, rings are literal.

  * ``StepStreamQ8``     one ``step`` per chunk of ``stride`` frames, literal int8 rings (the interpreter's ``invoke``)
  * ``whole_sequence``   the vectorised form: each layer's input left-padded with its ring (zero-point rows from reset)
  * ``non_stream``       the non-streaming model (valid layers, the residual right-aligned) on the windows ending at T, T + s, ...
Outputs are uint8; the probability is float32(u8) * float32(1/255).
"""
from __future__ import annotations

import math

import numpy as np

import quant_oracle as qo
from quant_oracle import INV255, imatmul, quantize_input, requant  # noqa: F401  (the plain MixedNet restatement's cells)

LEFT_SHIFT = 20


def quantize_multiplier(m):
    """QuantizeMultiplier restated: m = M * 2^(shift - 31), M in [2^30, 2^31)"""
    if m == 0.0:
        return 0, 0
    q, shift = math.frexp(float(m))
    M = int(math.floor(q * (1 << 31) + 0.5))
    if M == 1 << 31:
        M, shift = M // 2, shift + 1
    return (0, 0) if shift < -31 else (M, shift)


def add_multipliers(s1, s2, s_out):
    """(M1, sh1, M2, sh2, Mo, sho) of TFLite's int8 Add from the float32 scales, in double"""
    s1, s2, s_out = (float(np.float32(v)) for v in (s1, s2, s_out))
    twice_max = 2.0 * max(s1, s2)
    out = []
    for m in (s1 / twice_max, s2 / twice_max, twice_max / ((1 << LEFT_SHIFT) * s_out)):
        out += list(quantize_multiplier(m))
    return tuple(out)


def mbqm_lt1(x, M, shift):
    """MultiplyByQuantizedMultiplierSmallerThanOneExp: RoundingDivideByPOT(SaturatingRoundingDoublingHighMul(x, M), -shift)"""
    assert shift <= 0
    return qo.rdpot(qo.srdhm(x, M), -shift)


def add_q8(q1, z1, q2, z2, mult, z_out, relu=True, input_rounding=True):
    """reference_integer_ops::AddElementwise with left_shift 20 on int arrays (or ints); the fused ReLU is the clamp's floor.
    ``input_rounding=False`` is NOT the contract: the two scaled inputs shifted without RoundingDivideByPOT's rounding term, for
    the condition that a case can tell the two apart."""
    M1, sh1, M2, sh2, Mo, sho = (int(v) for v in mult)
    scaled = mbqm_lt1 if input_rounding else (lambda x, M, sh: np.asarray(qo.srdhm(x, M), np.int64) >> -sh)
    a = scaled((np.asarray(q1, np.int64) - z1) << LEFT_SHIFT, M1, sh1)
    b = scaled((np.asarray(q2, np.int64) - z2) << LEFT_SHIFT, M2, sh2)
    raw = mbqm_lt1(a + b, Mo, sho) + z_out
    return np.clip(raw, max(-128, z_out) if relu else -128, 127).astype(np.int64)


def avg_pool_round(acc, n):
    """acc > 0 ? (acc + n / 2) / n : (acc - n / 2) / n with C's truncating division, clamped to int8"""
    acc = np.asarray(acc, np.int64)
    h = n // 2
    v = np.where(acc > 0, (acc + h) // n, -((h - acc) // n))
    return np.clip(v, -128, 127)


class Q:
    """the parameters as int64 arrays and the layer list"""

    def __init__(self, qm):
        self.qm = qm
        d = qm.desc
        self.k1, self.s = int(d["conv1_kernel"]), int(d["stride"])
        self.r1 = max(0, self.k1 - self.s)
        self.zp = [int(z) for z in qm.zero_points]
        self.scales = qm.scales
        self.scale0 = np.float32(qm.scales[0])
        self.ops = [dict(op, weights=op["weights"].astype(np.int64), bias=op["bias"].astype(np.int64)) for op in qm.ops]
        self.layers = self.ops[1:-1]
        self.dense = self.ops[-1]
        self.tf = int(d["t_final"])
        self.pool = {0: 0, "average": 1, "max": 2}[d["pool"]]
        self.t_final_map = self.dense["tensors"][0]   # the tensor under the head ring
        self.lut = qm.lut

    def conv1(self, x):
        return qo.Q.conv1(self, x)                    # conv1 is the plain restatement's

    def linear(self, op, x, relu):
        t_in, t_out = op["tensors"]
        return requant(imatmul(x - self.zp[t_in], op["weights"]) + op["bias"], op, self.zp[t_out], relu)

    def mix(self, op, x):
        """valid over the (already padded) rows x [n, C] -> [n - K + 1, C]"""
        t_in, t_out = op["tensors"]
        w = op["weights"]
        K = w.shape[0]
        n = x.shape[0] - K + 1
        acc = np.zeros((max(n, 0), w.shape[1]), np.int64) + op["bias"]
        for j in range(K):
            acc += (x[j:j + n] - self.zp[t_in]) * w[j]
        return requant(acc, op, self.zp[t_out], False)

    def pw_add(self, op, x, r, add_trace=None):
        t1, t2, to = op["add_tensors"]
        q1 = self.linear(op, x, False)
        mult = add_multipliers(self.scales[t1], self.scales[t2], self.scales[to])
        out = add_q8(q1, self.zp[t1], r, self.zp[t2], mult, self.zp[to])
        if add_trace is not None:
            add_trace.append((q1, r, out, self.zp[to], self.zp[t1], self.zp[t2], mult))
        return out

    def head(self, h, pool_trace=None):
        """h [n + tf - 1, C] (ring + map) -> int8 logits [n]"""
        zi = self.zp[self.t_final_map]
        w = self.dense["weights"]
        n = h.shape[0] - self.tf + 1
        if n <= 0:
            return np.zeros(0, np.int64)
        if self.pool:
            win = np.lib.stride_tricks.sliding_window_view(h, self.tf, axis=0)[:n]   # [n, C, tf]
            if self.pool == 1:
                acc = win.sum(axis=2)
                if pool_trace is not None:
                    pool_trace.append(acc)
                v = avg_pool_round(acc, self.tf)
            else:
                v = win.max(axis=2)
            acc = imatmul(v - zi, w[0]) + self.dense["bias"][0]
        else:
            acc = np.zeros(n, np.int64) + self.dense["bias"][0]
            for t in range(self.tf):
                acc += imatmul(h[t:t + n] - zi, w[t])
        return requant(acc, self.dense, self.zp[-1], False)

    def output(self, logit):
        u8 = self.lut[np.asarray(logit, np.int64) + 128].astype(np.uint8)
        return u8, u8.astype(np.float32) * INV255


def whole_sequence(qm, frames, trace=None, add_trace=None, pool_trace=None):
    """From reset over the fed frames [0, floor(L/s)*s) -> (uint8 [n], int8 logits [n], rings int8 flat in the layout of
    mww_stream_get_state after the call).  ``trace`` receives (relu, zero point, values) of every tensor that feeds a ring (each
    MixConv's input, the head's input); ``add_trace`` (1x1 output, r, ADD output, zp_out, zp_1, zp_2,
    multipliers) of every ADD; ``pool_trace`` the
    average pool's int accumulators."""
    q = Q(qm)
    F = (len(frames) // q.s) * q.s
    n = F // q.s
    x = np.concatenate([np.full((q.r1, 40), q.zp[0], np.int64), quantize_input(np.asarray(frames[:F], np.float32), q.scale0, q.zp[0])], 0)
    rings = [x[x.shape[0] - q.r1:].reshape(-1)] if q.r1 else []
    a = q.conv1(x)[:n]
    relu, r = True, None
    for op in q.layers:
        if op["kind"] == "res":
            r = q.linear(op, a, False)            # [n, F]: index i is position i; no ring
        elif op["kind"] == "mix":
            R = op["weights"].shape[0] - 1
            zi = q.zp[op["tensors"][0]]
            a = np.concatenate([np.full((R, a.shape[1]), zi, np.int64), a], 0)
            rings.append(a[a.shape[0] - R:].reshape(-1))
            if trace is not None:
                trace.append((relu, zi, a[R:]))
            a, relu = q.mix(op, a), False
        elif op["kind"] == "pw":
            a, relu = q.linear(op, a, True), True
        else:
            a, relu = q.pw_add(op, a, r, add_trace), True
    zi = q.zp[q.t_final_map]
    if trace is not None:
        trace.append((relu, zi, a))
    h = np.concatenate([np.full((q.tf - 1, a.shape[1]), zi, np.int64), a], 0)
    if q.tf > 1:
        rings.append(h[h.shape[0] - (q.tf - 1):].reshape(-1))
    logit = q.head(h, pool_trace)
    u8, _ = q.output(logit)
    return u8, logit.astype(np.int8), np.concatenate(rings + [np.zeros(0, np.int64)]).astype(np.int8)


class StepStreamQ8:
    """literal rings, one call per chunk of ``stride`` frames"""

    def __init__(self, qm):
        self.q = Q(qm)
        self.reset()

    def reset(self):
        q = self.q
        self.ring1 = np.full((q.r1, 40), q.zp[0], np.int64)
        self.rings = {}
        for li, op in enumerate(q.layers):
            if op["kind"] == "mix":
                K, C = op["weights"].shape
                self.rings[li] = np.full((K - 1, C), q.zp[op["tensors"][0]], np.int64)
        self.hring = np.full((q.tf - 1, q.dense["weights"].shape[1]), q.zp[q.t_final_map], np.int64)

    def state(self):
        parts = ([self.ring1.reshape(-1)] if self.q.r1 else []) + [self.rings[k].reshape(-1) for k in sorted(self.rings)]
        if self.q.tf > 1:
            parts.append(self.hring.reshape(-1))
        return np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int8)

    def step(self, chunk):
        q = self.q
        mem = np.concatenate([self.ring1, quantize_input(chunk, q.scale0, q.zp[0])], 0)
        if q.r1:
            self.ring1 = mem[-q.r1:]
        x = q.conv1(mem)
        assert x.shape[0] == 1
        r = None
        for li, op in enumerate(q.layers):
            if op["kind"] == "res":
                r = q.linear(op, x, False)        # the current frame of the block input
            elif op["kind"] == "mix":
                mem = np.concatenate([self.rings[li], x], 0)
                self.rings[li] = mem[-(op["weights"].shape[0] - 1):]
                x = q.mix(op, mem)
                assert x.shape[0] == 1
            elif op["kind"] == "pw":
                x = q.linear(op, x, True)
            else:
                x = q.pw_add(op, x, r)
        mem = np.concatenate([self.hring, x], 0)
        if q.tf > 1:
            self.hring = mem[-(q.tf - 1):]
        return q.head(mem)[0]

    def run(self, frames):
        """-> (uint8 outputs, int8 logits)"""
        s = self.q.s
        logit = np.array([self.step(np.asarray(frames[i:i + s], np.float32)) for i in range(0, (len(frames) // s) * s, s)], np.int64)
        return self.q.output(logit)[0], logit.astype(np.int8)


def non_stream(qm, frames, T, want_logits=False):
    """the non-streaming model (no rings; StridedDrop right-aligns the residual) on the windows ending at T, T + s, ... <= L"""
    q = Q(qm)
    L = len(frames)
    if L < T:
        return (np.zeros(0, np.uint8), np.zeros(0, np.int8)) if want_logits else np.zeros(0, np.uint8)
    a = q.conv1(quantize_input(np.asarray(frames, np.float32), q.scale0, q.zp[0]))
    r = None
    for op in q.layers:
        if op["kind"] == "res":
            r = q.linear(op, a, False)
        elif op["kind"] == "mix":
            a = q.mix(op, a)
        elif op["kind"] == "pw":
            a = q.linear(op, a, True)
        else:
            a = q.pw_add(op, a, r[r.shape[0] - a.shape[0]:])
    logit = q.head(a)
    n = (L - T) // q.s + 1
    u8 = q.output(logit[:n])[0]
    return (u8, logit[:n].astype(np.int8)) if want_logits else u8
