"""TEST INFRASTRUCTURE: NumPy int64 restatement of the int8 streaming conv/BN graph (the Inception contract in
INTEGRATION.md) from the parameters of a ``microwakeword_amd.quantize_graph.QuantizedGraphModel``, driven by its
description and written apart from the kernel: the zero point of every source is subtracted from its values (the kernel
folds it into the bias), requantization is the restatement of tests/quant_oracle.py, rings are literal.

  * ``StepStreamQ8``     one ``step`` per frame.  Stems and the head are ``use_one_step=True`` (a ring of k / T_f rows that
                         includes the current one: shift one out, append, convolve all of them); every other op with k > 1
                         keeps a ring of d(k - 1) rows of its own input, concatenates ring and input, keeps the last
                         d(k - 1) rows and runs valid (layers/stream.py:241-255).
  * ``whole_sequence``   the vectorised form: each stateful op's input left-padded with its ring (zero-point rows from
                         reset), every op valid and right-aligned; uint8 outputs, int8 logits, rings after the call.
  * ``non_stream``       the non-streaming model (no rings) on the windows ending at T, T + 1, ... <= L.
  * ``synthetic_quantized``  a QuantizedGraphModel of any description from random weights and fixed ranges.
Outputs are uint8; the probability is float32(u8) * float32(1/255).
"""
from __future__ import annotations

import numpy as np

from microwakeword_amd import quantize_graph as qg
from quant_oracle import INV255, imatmul, quantize_input, requant   # noqa: F401  (INV255 is part of this module's interface)


class Q:
    """the parameters as int64 arrays and the op list of the description"""

    def __init__(self, qm):
        self.qm = qm
        self.desc = qm.desc
        self.dops = qm.desc["conv_ops"]
        self.n = len(self.dops)
        self.names = qm.names[1:-1]
        self.sources = qg.op_sources(qm.desc)
        self.zp = [int(z) for z in qm.zero_points]
        self.scale0 = np.float32(qm.scales[0])
        self.ops = [dict(op, weights=op["weights"].astype(np.int64), bias=op["bias"].astype(np.int64)) for op in qm.ops]
        self.dense = self.ops[-1]
        self.tf, self.c_last = self.dense["weights"].shape
        self.lut = qm.lut
        self.R = [(int(o["kernel"]) - 1) * int(o.get("dilation", 1)) for o in self.dops]

    def gather(self, i, tensors, rows=None):
        """the concatenated input of op i from full tensors: its sources' slices, right-aligned to the shortest; raw int8"""
        parts = [tensors[t][:, c0:c0 + cn] for t, c0, cn in self.sources[i]]
        m = min(p.shape[0] for p in parts) if rows is None else rows
        return np.concatenate([p[p.shape[0] - m:] for p in parts], 1)

    def zp_row(self, i):
        """the zero point under every column of op i's concatenated input"""
        return np.concatenate([np.full(cn, self.zp[t], np.int64) for t, _, cn in self.sources[i]])

    def conv(self, i, mem):
        """op i valid over its (already padded) raw int8 input mem [n, Cin] -> [n - d(k - 1), Co]"""
        op, o = self.ops[i], self.dops[i]
        k, d = int(o["kernel"]), int(o.get("dilation", 1))
        w = op["weights"]                                    # [k, Cin, Co]
        m = mem.shape[0] - d * (k - 1)
        if m <= 0:
            return np.zeros((0, w.shape[2]), np.int64)
        x = mem - self.zp_row(i)[None, :]
        acc = np.zeros((m, w.shape[2]), np.int64) + op["bias"]
        for j in range(k):
            acc += imatmul(x[j * d:j * d + m], w[j])
        return requant(acc, op, self.zp[1 + i], True)

    def head(self, h):
        """Dense at every position of the padded final map h [n + tf - 1, C] -> int8 logits [n]"""
        w = self.dense["weights"]
        n = h.shape[0] - self.tf + 1
        acc = np.zeros(max(n, 0), np.int64) + self.dense["bias"][0]
        for t in range(self.tf):
            acc += imatmul(h[t:t + n] - self.zp[self.n], w[t])
        return requant(acc, self.dense, self.zp[-1], False)

    def output(self, logit):
        u8 = self.lut[np.asarray(logit, np.int64) + 128].astype(np.uint8)
        return u8, u8.astype(np.float32) * INV255


def whole_sequence(qm, frames, trace=None):
    """From reset over ``frames`` [N, 40] -> (uint8 [N], int8 logits [N], rings int8 flat in the layout of
    mww_stream_get_state after the call).  ``trace``: a list that receives (relu, zero point, values) of every activation
    tensor that feeds a ring (a source of an op with k > 1 other than the spectrogram; the head's input)."""
    q = Q(qm)
    x = quantize_input(np.asarray(frames, np.float32).reshape(-1, 40), q.scale0, q.zp[0])
    N = x.shape[0]
    tensors, rings, traced = [x], [], set()
    for i in range(q.n):
        a = q.gather(i, tensors)
        assert a.shape[0] == N
        R = q.R[i]
        if R:
            a = np.concatenate([np.tile(q.zp_row(i), (R, 1)), a], 0)
            rings.append(a[a.shape[0] - R:].reshape(-1))
            if trace is not None:
                for t, _, _ in q.sources[i]:
                    if t > 0 and t not in traced:
                        traced.add(t)
                        trace.append((True, q.zp[t], tensors[t]))
        tensors.append(q.conv(i, a))
    last = tensors[-1]
    if trace is not None and q.n not in traced:
        trace.append((True, q.zp[q.n], last))
    h = np.concatenate([np.full((q.tf - 1, q.c_last), q.zp[q.n], np.int64), last], 0)
    if q.tf > 1:
        rings.append(h[h.shape[0] - (q.tf - 1):].reshape(-1))
    logit = q.head(h)
    u8, _ = q.output(logit)
    return u8, logit.astype(np.int8), np.concatenate(rings + [np.zeros(0, np.int64)]).astype(np.int8)


class StepStreamQ8:
    """literal rings, one call per frame"""

    def __init__(self, qm):
        self.q = Q(qm)
        self.reset()

    def one_step(self, i):
        return self.q.names[i].startswith("stem")

    def reset(self):
        q = self.q
        self.rings = {}
        for i in range(q.n):
            if q.R[i]:
                rows = q.R[i] + 1 if self.one_step(i) else q.R[i]
                self.rings[i] = np.tile(q.zp_row(i), (rows, 1))
        self.hring = np.full((q.tf, q.c_last), q.zp[q.n], np.int64)   # use_one_step=True: T_f rows including the current one

    def state(self):
        q = self.q
        parts = [(self.rings[i][1:] if self.one_step(i) else self.rings[i]).reshape(-1) for i in sorted(self.rings)]
        if q.tf > 1:
            parts.append(self.hring[1:].reshape(-1))
        return np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int8)

    def step(self, frame):
        q = self.q
        tensors = [quantize_input(np.asarray(frame, np.float32).reshape(1, 40), q.scale0, q.zp[0])]
        for i in range(q.n):
            x = q.gather(i, tensors)
            assert x.shape[0] == 1
            if q.R[i] == 0:
                mem = x
            elif self.one_step(i):
                mem = self.rings[i] = np.concatenate([self.rings[i][1:], x], 0)
            else:
                mem = np.concatenate([self.rings[i], x], 0)
                self.rings[i] = mem[mem.shape[0] - q.R[i]:]
            y = q.conv(i, mem)
            assert y.shape[0] == 1
            tensors.append(y)
        self.hring = np.concatenate([self.hring[1:], tensors[-1]], 0)
        return q.head(self.hring)[0]

    def run(self, frames):
        logit = np.array([self.step(f) for f in np.asarray(frames, np.float32).reshape(-1, 40)], np.int64)
        return self.q.output(logit)[0], logit.astype(np.int8)


def non_stream(qm, frames, T, want_logits=False):
    """the non-streaming model on the windows ending at T, T + 1, ... <= L -> uint8 (and the int8 logits)"""
    q = Q(qm)
    L = len(frames)
    if L < T:
        return (np.zeros(0, np.uint8), np.zeros(0, np.int8)) if want_logits else np.zeros(0, np.uint8)
    tensors = [quantize_input(np.asarray(frames, np.float32).reshape(-1, 40), q.scale0, q.zp[0])]
    for i in range(q.n):
        tensors.append(q.conv(i, q.gather(i, tensors)))
    logit = q.head(tensors[-1])
    # the description's receptive field is the window - or shorter, where a drop removes more leading frames than aligning
    # the sources needs: the ops run right-aligned, so the windows ending at T, T + 1, ... are the last L - T + 1 positions
    assert logit.size >= L - T + 1, (logit.size, L, T)
    logit = logit[logit.size - (L - T + 1):]
    u8 = q.output(logit)[0]
    return (u8, logit.astype(np.int8)) if want_logits else u8


def random_weights(desc, seed=0):
    """random Keras-order weights of a graph description (per op kernel, gamma, beta, moving mean, moving variance; dense)"""
    rng = np.random.default_rng(seed)
    w = []
    for o, srcs in zip(desc["conv_ops"], qg.op_sources(desc)):
        cin, k, co, g = sum(cn for _, _, cn in srcs), int(o["kernel"]), int(o["filters"]), int(o.get("bn_groups", 1))
        slots = g if g > 1 else co
        w += [rng.normal(0, 1.0 / np.sqrt(k * cin), (k, 1, cin, co)) * (0.15 if srcs[0][0] == 0 else 1.6), 1 + rng.random(slots),
              rng.normal(0.1, 0.1, slots), rng.normal(0, 0.1, slots), 1 + rng.random(slots)]
    return w


def final_frames(desc):
    """T_f of a description: the rows of the last op's output for a window of ``frames`` rows"""
    length = [int(desc["frames"])]
    for o in desc["conv_ops"]:
        drop = list(o.get("drop", [0] * len(o["src"])))
        tin = min(length[int(s) + 1] - int(d) for s, d in zip(o["src"], drop))
        length.append(tin - (int(o["kernel"]) - 1) * int(o.get("dilation", 1)))
    return length[-1]


def synthetic_quantized(desc, seed=0, ranges=None):
    """a QuantizedGraphModel of any graph description from random Keras-order weights and fixed ranges (descriptions no
    float model instantiates: fused branch heads read through channel slices, tiles too large for LDS); run it with the
    context of any float model.  ``ranges`` [n_ops + 2, 2] replaces the fixed ranges."""
    w = random_weights(desc, seed)
    rng = np.random.default_rng(seed + 1000)
    c_last = int(desc["conv_ops"][-1]["filters"])
    w += [rng.normal(0, 0.05, (final_frames(desc) * c_last, 1)), rng.normal(0, 0.1, 1)]
    if ranges is None:
        ranges = [(0.0, 26.0)] + [(0.0, 4.0)] * len(desc["conv_ops"]) + [(-8.0, 8.0)]
    return qg.quantize_weights(desc, w, np.array(ranges, np.float32))
