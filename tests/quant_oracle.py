"""TEST INFRASTRUCTURE: NumPy int64 restatement of the int8 streaming MixedNet (the contract in INTEGRATION.md) from the
parameters of a ``microwakeword_amd.quantize.QuantizedModel``, written apart from the kernel: the input zero point is
subtracted from every input (the kernel folds it into the bias), requantization is restated here, rings are literal.

  * ``StepStreamQ8``     one ``step`` per chunk of ``stride`` frames: every Stream layer concatenates its int8 ring with the
                         new input, keeps the last R rows as the new ring and runs valid (the interpreter's ``invoke``)
  * ``whole_sequence``   the vectorised form: each layer's input left-padded with its ring (zero-point rows from reset)
  * ``non_stream``       the non-streaming model on the windows ending at T, T + s, ... <= L
Outputs are uint8; the probability is float32(u8) * float32(1/255).
"""
from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INV255 = np.float32(1 / 255)


def srdhm(a, b):
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    ab = a * b
    v = ab + np.where(ab >= 0, np.int64(1 << 30), np.int64(1 - (1 << 30)))
    q = np.where(v >= 0, v >> 31, -((-v) >> 31))
    return np.where((a == INT32_MIN) & (b == INT32_MIN), INT32_MAX, q)


def rdpot(x, e):
    x = np.asarray(x, np.int64)
    e = np.asarray(e, np.int64)
    mask = (np.int64(1) << e) - 1
    r = x & mask
    t = (mask >> 1) + (x < 0)
    return (x >> e) + (r > t)


def wrap32(x):
    x = np.asarray(x, np.int64) & 0xFFFFFFFF
    return np.where(x >= (1 << 31), x - (1 << 32), x)


def mbqm(x, M, shift):
    shift = np.asarray(shift, np.int64)
    left, right = np.maximum(shift, 0), np.maximum(-shift, 0)
    return rdpot(srdhm(wrap32(np.asarray(x, np.int64) << left), M), right)


BRANCHES = None   # a set while ``record_branches`` is active: the requantization / input branches the ORACLE took


class record_branches:
    """``with record_branches() as seen:`` collects the names of the branches every ``requant`` / ``quantize_input`` of
    this module takes inside the block (the oracle is instrumented, never the kernel): rq-left-shift, rq-right-shift>=16,
    rq-shift=-31, rq-shift=+30, rq-clamp-low-relu, rq-clamp-low-norelu, rq-clamp-127, rq-zp-out=-128 / 0 / 127,
    in-sat-low, in-sat-high."""

    def __enter__(self):
        global BRANCHES
        self.prev, BRANCHES = BRANCHES, set()
        return BRANCHES

    def __exit__(self, *exc):
        global BRANCHES
        BRANCHES = self.prev
        return False


def requant(acc, op, zp_out, relu):
    lo = max(-128, zp_out) if relu else -128
    v = mbqm(acc, op["multiplier"], op["shift"]) + zp_out
    if BRANCHES is not None and np.size(acc):
        sh = np.asarray(op["shift"], np.int64)
        for name, hit in (("rq-left-shift", np.any(sh > 0)), ("rq-right-shift>=16", np.any(sh <= -16)),
                          ("rq-shift=-31", np.any(sh == -31)), ("rq-shift=+30", np.any(sh == 30)),
                          ("rq-clamp-low-relu" if relu else "rq-clamp-low-norelu", np.any(v < lo)),
                          ("rq-clamp-127", np.any(v > 127)), ("rq-zp-out=%d" % zp_out, zp_out in (-128, 0, 127))):
            if hit:
                BRANCHES.add(name)
    return np.clip(v, lo, 127).astype(np.int64)


def imatmul(a, b):
    """exact integer a @ b through float64: every partial sum of |int8 - zp| * |int8| terms stays below 2^53"""
    return np.rint(np.asarray(a, np.float64) @ np.asarray(b, np.float64)).astype(np.int64)


def quantize_input(x, scale, zp):
    """float32(x / scale) + float32(zp), truncated, saturated"""
    t = np.asarray(x, np.float32) / np.float32(scale) + np.float32(zp)
    if BRANCHES is not None and t.size:
        if np.any(np.trunc(t) < -128):
            BRANCHES.add("in-sat-low")
        if np.any(np.trunc(t) > 127):
            BRANCHES.add("in-sat-high")
    return np.clip(np.trunc(t), -128, 127).astype(np.int64)


class Q:
    """the parameters as int64 arrays, and the layer list"""

    def __init__(self, qm):
        self.qm = qm
        d = qm.desc
        self.k1, self.s = int(d["conv1_kernel"]), int(d["stride"])
        self.r1 = max(0, self.k1 - self.s)
        self.zp = [int(z) for z in qm.zero_points]
        self.scale0 = np.float32(qm.scales[0])
        self.ops = [dict(op, weights=op["weights"].astype(np.int64), bias=op["bias"].astype(np.int64)) for op in qm.ops]
        self.layers = self.ops[1:-1]
        self.dense = self.ops[-1]
        self.tf = self.dense["weights"].shape[0]
        self.lut = qm.lut

    def conv1(self, x):
        """valid, stride s over int8 rows x [n, 40] -> [m, C1]"""
        op = self.ops[0]
        m = (x.shape[0] - self.k1) // self.s + 1
        w = op["weights"]                                   # [k1*40, C1]
        if m <= 0:
            return np.zeros((0, w.shape[1]), np.int64)
        acc = np.zeros((m, w.shape[1]), np.int64) + op["bias"]
        for k in range(self.k1):   # tap k of output i reads row i * s + k
            acc += imatmul(x[k:k + (m - 1) * self.s + 1:self.s] - self.zp[0], w[k * 40:(k + 1) * 40])
        return requant(acc, op, self.zp[1], True)

    def layer(self, li, x):
        """layer li on its (already padded) int8 input x [n, C]: mix valid -> [n - K + 1, C]; pw -> [n, Co]"""
        op = self.layers[li]
        zi, zo = self.zp[1 + li], self.zp[2 + li]
        w = op["weights"]
        if op["kind"] == "mix":
            K = w.shape[0]
            n = x.shape[0] - K + 1
            acc = np.zeros((max(n, 0), w.shape[1]), np.int64) + op["bias"]
            for j in range(K):
                acc += (x[j:j + n] - zi) * w[j]
            return requant(acc, op, zo, False)
        return requant(imatmul(x - zi, w) + op["bias"], op, zo, True)

    def head(self, h):
        """Dense at every position of the padded final map h [n + tf - 1, C] -> int8 logits [n]"""
        w = self.dense["weights"]                            # [tf, C]
        zi = self.zp[1 + len(self.layers)]
        n = h.shape[0] - self.tf + 1
        acc = np.zeros(max(n, 0), np.int64) + self.dense["bias"][0]
        for t in range(self.tf):
            acc += imatmul(h[t:t + n] - zi, w[t])
        return requant(acc, self.dense, self.zp[-1], False)

    def output(self, logit):
        u8 = self.lut[np.asarray(logit, np.int64) + 128].astype(np.uint8)
        return u8, u8.astype(np.float32) * INV255


def whole_sequence(qm, frames, trace=None):
    """From reset over the fed frames [0, floor(L/s)*s) -> (uint8 [n], int8 logits [n], rings int8 flat in the layout of
    mww_stream_get_state after the call).  ``trace``: a list that receives (relu, zero point, values) of every activation
    tensor that feeds a ring (each MixConv's input, the head's input)."""
    q = Q(qm)
    F = (len(frames) // q.s) * q.s
    n = F // q.s
    x = np.concatenate([np.full((q.r1, 40), q.zp[0], np.int64), quantize_input(np.asarray(frames[:F], np.float32), q.scale0, q.zp[0])], 0)
    rings = [x[x.shape[0] - q.r1:].reshape(-1)] if q.r1 else []
    a = q.conv1(x)[:n]
    for li, op in enumerate(q.layers):
        if op["kind"] == "mix":
            R = op["weights"].shape[0] - 1
            a = np.concatenate([np.full((R, a.shape[1]), q.zp[1 + li], np.int64), a], 0)
            rings.append(a[a.shape[0] - R:].reshape(-1))
            if trace is not None:   # a MixConv input is conv1's or a pointwise layer's output (ReLU) unless a MixConv precedes it
                trace.append((li == 0 or q.layers[li - 1]["kind"] == "pw", q.zp[1 + li], a[R:]))
        a = q.layer(li, a)
    if trace is not None:
        trace.append((True, q.zp[1 + len(q.layers)], a))
    h = np.concatenate([np.full((q.tf - 1, a.shape[1]), q.zp[1 + len(q.layers)], np.int64), a], 0)
    if q.tf > 1:
        rings.append(h[h.shape[0] - (q.tf - 1):].reshape(-1))
    logit = q.head(h)
    u8, _ = q.output(logit)
    st = np.concatenate(rings + [np.zeros(0, np.int64)]).astype(np.int8)
    return u8, logit.astype(np.int8), st


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
                self.rings[li] = np.full((op["weights"].shape[0] - 1, op["weights"].shape[1]), q.zp[1 + li], np.int64)
        c = q.dense["weights"].shape[1]
        self.hring = np.full((q.tf - 1, c), q.zp[1 + len(q.layers)], np.int64)

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
        for li, op in enumerate(q.layers):
            if op["kind"] == "mix":
                mem = np.concatenate([self.rings[li], x], 0)
                self.rings[li] = mem[-(op["weights"].shape[0] - 1):]
                x = q.layer(li, mem)
                assert x.shape[0] == 1
            else:
                x = q.layer(li, x)
        mem = np.concatenate([self.hring, x], 0)
        if q.tf > 1:
            self.hring = mem[-(q.tf - 1):]
        return q.head(mem)[0]

    def run(self, frames):
        s = self.q.s
        logit = np.array([self.step(np.asarray(frames[i:i + s], np.float32)) for i in range(0, (len(frames) // s) * s, s)], np.int64)
        return self.q.output(logit)[0]


def non_stream(qm, frames, T, want_logits=False):
    """the non-streaming model (no rings) on the windows ending at T, T + s, ... <= L -> uint8 (and the int8 logits)"""
    q = Q(qm)
    L = len(frames)
    if L < T:
        return (np.zeros(0, np.uint8), np.zeros(0, np.int8)) if want_logits else np.zeros(0, np.uint8)
    a = q.conv1(quantize_input(np.asarray(frames, np.float32), q.scale0, q.zp[0]))
    for li in range(len(q.layers)):
        a = q.layer(li, a)
    logit = q.head(a)
    n = (L - T) // q.s + 1
    u8 = q.output(logit[:n])[0]
    return (u8, logit[:n].astype(np.int8)) if want_logits else u8
