"""TEST INFRASTRUCTURE: float64 (and float32) restatements of the streaming MixedNet with residual connections and a pooled
head (Modes.STREAM_INTERNAL_STATE_INFERENCE; mixednet.py:340-358, :362-381) from the Keras-order weights of
``oracle.model_oracle.OracleModel``, next to tests/streaming_oracle.py whose conv1 / MixConv / 1x1 cells they reuse.

  * residual   ``r = BN_res(Conv1x1_res(block input))`` has no Stream wrapper: no ring, no state.  It is added to the BN output
               of every repeat of the block before the ReLU.  In stream mode StridedDrop is the identity and both branches
               hold the current frame; in the whole-sequence form every Stream layer keeps the length of its input (it is
               left-padded with its ring), so equal indices are equal positions.
  * pooled     the head's Stream(Identity) keeps T_f - 1 frames; Average / MaxPooling2D((T_f, 1)) runs over the ring plus the
               current frame (cold zeros take part), the Dense over the C pooled values.
  * ``StepStream``      literal ring buffers, one call per chunk of ``stride`` frames
  * ``whole_sequence``  the vectorised form from zero state
The non_stream windows (spatial attention included) go through ``OracleModel.predict_with_logits``
(``streaming_oracle.non_stream_windows``).  ``StepStream.state()`` and ``whole_sequence(..., rings=True)`` give the rings in
the layout of mww_stream_get_state: conv1, every MixConv in layer order, the head [T_f - 1][C].
"""
from __future__ import annotations

import numpy as np

from oracle import model_oracle as mo
import streaming_oracle as so


def t_final_of(flags, T):
    """frames of the final map before attention and pooling"""
    k1, s = int(flags["first_conv_kernel_size"]), int(flags["stride"])
    t = (T - k1) // s + 1
    for r, ks in zip(mo.parse(flags["repeat_in_block"]), mo.parse(flags["mixconv_kernel_sizes"])):
        ks = list(ks) if isinstance(ks, (list, tuple)) else [ks]
        t -= int(r) * (max(ks) - 1)
    return t


class Net(so.Net):
    """``T``: the window of the non-streaming model the weights belong to (it fixes T_f, which a pooled Dense does not show)"""

    def __init__(self, flags, om, T, dtype=np.float64, body_only=False):
        """``body_only``: the layers in front of the head only (a dry run that conditions the weights of any flag set)"""
        super().__init__(flags, om, dtype)
        self.tf = t_final_of(flags, T)
        assert body_only or not (flags.get("spatial_attention") and self.tf > 1), "no streaming form of spatial attention is restated"
        self.pool = (2 if flags.get("max_pool") else 1) if flags.get("pooled") and self.tf > 1 else 0
        res = [int(bool(r)) for r in mo.parse(flags["residual_connection"])]
        # the layer list of streaming_oracle.Net with ("res", "b<i>", None) in front of a residual block's repeats; a 1x1 layer
        # of such a block is ("pw", "b<i>.r<j>", "b<i>"): the third entry names the residual it adds
        self.layers = []
        pf, rep = mo.parse(flags["pointwise_filters"]), mo.parse(flags["repeat_in_block"])
        for bi, (f, r, ks) in enumerate(zip(pf, rep, mo.parse(flags["mixconv_kernel_sizes"]))):
            ks = list(ks) if isinstance(ks, (list, tuple)) else [ks]
            if res[bi]:
                self.layers.append(("res", "b%d" % bi, None))
            for ri in range(r):
                p = "b%d.r%d" % (bi, ri)
                if max(ks) > 1:
                    self.layers.append(("mix", p, ks))
                self.layers.append(("pw", p, "b%d" % bi if res[bi] else None))
        assert body_only or self.wd.size == (1 if self.pool else self.tf) * self.c_last

    def _bn(self, y, p):
        g, b = self.w[p + ".gamma"], self.w[p + ".beta"]
        mu, var = self.w[p + ".moving_mean"], self.w[p + ".moving_variance"]
        return (y - mu) / np.sqrt(var + self.dtype.type(so.BN_EPS)) * g + b

    def res(self, b, x):
        """the residual branch of block ``b`` on its input x [n, Cin] -> [n, F] (linear)"""
        return self._bn(x @ self.w[b + ".res.kernel"][0, 0], b + ".res.bn")

    def pw_res(self, p, x, r):
        """1x1 + BN (+ residual) + ReLU"""
        y = self._bn(x @ self.w[p + ".pw.kernel"][0, 0], p + ".bn")
        return np.maximum(y if r is None else y + r, 0)

    def head(self, mem):
        """mem [T_f, C] (ring + current frame) -> logit"""
        if self.pool:
            v = mem.sum(axis=0) / self.dtype.type(self.tf) if self.pool == 1 else mem.max(axis=0)
            return v @ self.wd + self.bd
        return mem.reshape(-1) @ self.wd + self.bd

    def ring_sizes_flat(self):
        out, c = [self.r1 * 40], self.w["conv1.kernel"].shape[3]
        for kind, p, ks in self.layers:
            if kind == "mix":
                out.append((max(ks) - 1) * c)
            elif kind == "pw":
                c = self.w[p + ".pw.kernel"].shape[3]
        return out + [(self.tf - 1) * self.c_last]


class StepStream:
    """One ``step`` per chunk of ``stride`` frames (the streaming interpreter's ``invoke``), literal ring buffers."""

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
            elif kind == "pw":
                c = n.w[p + ".pw.kernel"].shape[3]
        self.hring = np.zeros((n.tf - 1, n.c_last), n.dtype)

    def state(self):
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
        r = {}
        for kind, p, ks in n.layers:
            if kind == "res":
                r[p] = n.res(p, x)     # the current frame of the block input; no ring
            elif kind == "mix":
                mem = np.concatenate([self.rings[p], x], 0)
                self.rings[p] = mem[-(max(ks) - 1):]
                x = n.mix(p, ks, mem)
                assert x.shape[0] == 1
            else:
                x = n.pw_res(p, x, r[ks] if ks else None)
        mem = np.concatenate([self.hring, x], 0)
        if n.tf > 1:
            self.hring = mem[-(n.tf - 1):]
        return n.head(mem)

    def run(self, frames):
        s = self.net.s
        return np.array([self.step(frames[i:i + s]) for i in range(0, (len(frames) // s) * s, s)])


def whole_sequence(net: Net, frames, rings=False):
    """Vectorised streaming form from zero state over the fed frames [0, floor(L/s)*s) -> logits [floor(L/s)]; with
    ``rings`` also the state after those frames, flat, in the layout of mww_stream_get_state."""
    s, dt = net.s, net.dtype
    F = (len(frames) // s) * s
    if F == 0:
        z = np.zeros(0, dt)
        return (z, np.zeros(sum(net.ring_sizes_flat()), dt)) if rings else z
    x = np.concatenate([np.zeros((net.r1, 40), dt), np.asarray(frames[:F], dt)], 0)
    st = [x[x.shape[0] - net.r1:].reshape(-1)]
    a = net.conv1(x)
    n = F // s
    assert a.shape[0] == n
    r = {}
    for kind, p, ks in net.layers:
        if kind == "res":
            r[p] = net.res(p, a)       # [n, F]: index i is position i, as in every layer below (each keeps the length n)
        elif kind == "mix":
            R = max(ks) - 1
            a = np.concatenate([np.zeros((R, a.shape[1]), dt), a], 0)
            st.append(a[a.shape[0] - R:].reshape(-1))
            a = net.mix(p, ks, a)
        else:
            a = net.pw_res(p, a, r[ks] if ks else None)
        assert a.shape[0] == n
    h = np.concatenate([np.zeros((net.tf - 1, a.shape[1]), dt), a], 0)
    st.append(h[h.shape[0] - (net.tf - 1):].reshape(-1))
    win = np.lib.stride_tricks.sliding_window_view(h, net.tf, axis=0)[:n]   # [n, C, tf]
    if net.pool:
        # the frames in order, as the literal form sums them
        v = (np.add.reduce(np.moveaxis(win, 2, 0), axis=0) / dt.type(net.tf)) if net.pool == 1 else win.max(axis=2)
        z = v @ net.wd + net.bd
    else:
        z = np.einsum("nct,tc->n", win, net.wd.reshape(net.tf, -1)) + net.bd
    return (z, np.concatenate(st)) if rings else z
