"""TEST INFRASTRUCTURE: float64 restatements of the streaming MixedNet (Modes.STREAM_INTERNAL_STATE_INFERENCE) from the
Keras-order weights of ``oracle.model_oracle.OracleModel``.

  * ``StepStream``   literal ring buffers, one call per chunk of ``stride`` frames: every Stream layer concatenates its
                     ring with the new input, keeps the last R frames as the new ring and applies its cell with valid
                     padding (microwakeword/layers/stream.py:580-594); conv1 R = max(0, k1 - s) (stream.py:247-255),
                     MixConv R = max(ks) - 1 with StridedKeep(ks) per group (mixednet.py:193-231, strided_drop.py), the
                     head's Stream(Identity) R = T_f - 1 (mixednet.py:365-373); BN with the moving statistics.
  * ``whole_sequence``  the vectorised form: each Stream layer's input left-padded with its R state frames, every layer
                     valid and right-aligned, the Dense at every position of the final map.
  * ``non_stream_windows``  the non-streaming model on the windows ending at T, T + s, ... <= L.
``Net(..., dtype=np.float32)`` runs the same restatement in float32 (its distance from the float64 form is the rounding a
float32 implementation of these sums carries: tests/stream_sweep.py conditions its inputs on it).  ``StepStream.state()`` and
``whole_sequence(..., rings=True)`` give the rings in the layout of mww_stream_get_state.
"""
from __future__ import annotations

import numpy as np

from oracle import model_oracle as mo

BN_EPS = 1e-3


class Net:
    def __init__(self, flags, om, dtype=np.float64):
        self.flags = flags
        self.dtype = np.dtype(dtype)
        w = {v.name: np.asarray(v.value, self.dtype) for v in om.vars}
        self.w = w
        self.k1, self.s = int(flags["first_conv_kernel_size"]), int(flags["stride"])
        self.r1 = max(0, self.k1 - self.s)
        self.layers = []
        pf, rep = mo.parse(flags["pointwise_filters"]), mo.parse(flags["repeat_in_block"])
        ksz = mo.parse(flags["mixconv_kernel_sizes"])
        for bi, (f, r, ks) in enumerate(zip(pf, rep, ksz)):
            ks = list(ks) if isinstance(ks, (list, tuple)) else [ks]
            for ri in range(r):
                p = "b%d.r%d" % (bi, ri)
                if max(ks) > 1:
                    self.layers.append(("mix", p, ks))
                self.layers.append(("pw", p, None))
        self.wd = w["dense.kernel"][:, 0]
        self.bd = w["dense.bias"][0]
        self.c_last = int(pf[-1])
        self.tf = self.wd.size // self.c_last

    def conv1(self, mem):
        """valid, stride s over mem [n, 40] -> [m, C1] (ReLU)"""
        k = self.w["conv1.kernel"][:, 0]   # [k1, 40, C1]
        m = (mem.shape[0] - self.k1) // self.s + 1
        if m <= 0:
            return np.zeros((0, k.shape[2]), self.dtype)
        win = np.lib.stride_tricks.sliding_window_view(mem, self.k1, axis=0)[::self.s][:m]   # [m, 40, k1]
        return np.maximum(np.einsum("mbk,kbc->mc", win, k), 0)

    def mix(self, p, ks, mem):
        """MixConv on mem [n, C]: groups right-aligned (StridedKeep / StridedDrop), valid -> [n - max(ks) + 1, C]"""
        C = mem.shape[1]
        groups = mo.split_channels(C, len(ks)) if len(ks) > 1 else [C]
        K = max(ks)
        n = mem.shape[0] - K + 1
        outs, c0 = [], 0
        for gi, (gc, k) in enumerate(zip(groups, ks)):
            kern = self.w["%s.dw%d.kernel" % (p, gi)][:, 0, :, 0]   # [k, gc]
            x = mem[K - k:, c0:c0 + gc]
            win = np.lib.stride_tricks.sliding_window_view(x, k, axis=0)[:n]   # [n, gc, k]
            o = np.einsum("ngk,kg->ng", win, kern) + self.w["%s.dw%d.bias" % (p, gi)]
            outs.append(o)
            c0 += gc
        return np.concatenate(outs, axis=1)

    def pw(self, p, x):
        y = x @ self.w[p + ".pw.kernel"][0, 0]
        g, b = self.w[p + ".bn.gamma"], self.w[p + ".bn.beta"]
        mu, var = self.w[p + ".bn.moving_mean"], self.w[p + ".bn.moving_variance"]
        return np.maximum((y - mu) / np.sqrt(var + self.dtype.type(BN_EPS)) * g + b, 0)

    def ring_sizes(self):
        return [self.r1] + [max(ks) - 1 for kind, _, ks in self.layers if kind == "mix"] + [self.tf - 1]

    def ring_sizes_flat(self):
        """elements of every ring in state order: conv1 [r1, 40], each MixConv [K - 1, C_in], the head [tf - 1, C_last]"""
        out, c = [self.r1 * 40], self.w["conv1.kernel"].shape[3]
        for kind, p, ks in self.layers:
            if kind == "mix":
                out.append((max(ks) - 1) * c)
            else:
                c = self.w[p + ".pw.kernel"].shape[3]
        return out + [(self.tf - 1) * self.c_last]


class StepStream:
    """One ``step`` per chunk of ``stride`` frames (the streaming interpreter's ``invoke``)."""

    def __init__(self, net: Net):
        self.net = net
        self.reset()

    def reset(self):
        n = self.net
        self.ring1 = np.zeros((n.r1, 40), n.dtype)
        self.rings = {}
        c = n.w["conv1.kernel"].shape[3]
        for kind, p, ks in n.layers:
            if kind == "mix":
                self.rings[p] = np.zeros((max(ks) - 1, c), n.dtype)
            else:
                c = n.w[p + ".pw.kernel"].shape[3]
        self.hring = np.zeros((n.tf - 1, n.c_last), n.dtype)

    def state(self):
        """the rings, flat, in the layout of mww_stream_get_state: conv1, every MixConv in layer order, the head"""
        n = self.net
        parts = [self.ring1.reshape(-1)] + [self.rings[p].reshape(-1) for kind, p, _ in n.layers if kind == "mix"]
        return np.concatenate(parts + [self.hring.reshape(-1)])

    def step(self, chunk):
        n = self.net
        mem = np.concatenate([self.ring1, np.asarray(chunk, n.dtype)], 0)
        if n.r1:
            self.ring1 = mem[-n.r1:]
        x = n.conv1(mem)
        assert x.shape[0] == 1
        for kind, p, ks in n.layers:
            if kind == "mix":
                mem = np.concatenate([self.rings[p], x], 0)
                self.rings[p] = mem[-(max(ks) - 1):]
                x = n.mix(p, ks, mem)
                assert x.shape[0] == 1
            else:
                x = n.pw(p, x)
        mem = np.concatenate([self.hring, x], 0)
        if n.tf > 1:
            self.hring = mem[-(n.tf - 1):]
        z = mem.reshape(-1) @ n.wd + n.bd
        return z

    def run(self, frames):
        """predict_spectrogram: chunks of s, trailing L mod s frames dropped -> logits"""
        s = self.net.s
        return np.array([self.step(frames[i:i + s]) for i in range(0, (len(frames) // s) * s, s)])


def whole_sequence(net: Net, frames, state=None, rings=False):
    """Vectorised streaming form from zero state over the fed frames [0, floor(L/s)*s) -> logits [floor(L/s)]; with
    ``rings`` also the state after those frames (the last R rows of every Stream layer's padded input, flat, in the layout
    of mww_stream_get_state)."""
    s, dt = net.s, net.dtype
    F = (len(frames) // s) * s
    if F == 0:
        z = np.zeros(0, dt)
        return (z, np.zeros(sum(net.ring_sizes_flat()), dt)) if rings else z
    x = np.concatenate([np.zeros((net.r1, 40), dt), np.asarray(frames[:F], dt)], 0)
    st = [x[x.shape[0] - net.r1:].reshape(-1)]
    a = net.conv1(x)
    for kind, p, ks in net.layers:
        if kind == "mix":
            R = max(ks) - 1
            a = np.concatenate([np.zeros((R, a.shape[1]), dt), a], 0)
            st.append(a[a.shape[0] - R:].reshape(-1))
            a = net.mix(p, ks, a)
        else:
            a = net.pw(p, a)
    h = np.concatenate([np.zeros((net.tf - 1, a.shape[1]), dt), a], 0)
    st.append(h[h.shape[0] - (net.tf - 1):].reshape(-1))
    n = F // s
    W = net.wd.reshape(net.tf, -1)
    win = np.lib.stride_tricks.sliding_window_view(h, net.tf, axis=0)[:n]   # [n, C, tf]
    z = np.einsum("nct,tc->n", win, W) + net.bd
    return (z, np.concatenate(st)) if rings else z


def non_stream_windows(om, frames, T, s):
    """the non-streaming model on frames [e - T, e), e = T, T + s, ... <= L -> logits"""
    L = len(frames)
    if L < T:
        return np.zeros(0)
    x = np.stack([frames[e - T:e] for e in range(T, L + 1, s)])
    return om.predict_with_logits(x)[1]


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))
