"""TEST INFRASTRUCTURE: float64 restatements of the streaming Inception (Modes.STREAM_INTERNAL_STATE_INFERENCE of
microwakeword/inception.py:233-338, one spectrogram frame per step) from the Keras-order weights of
``oracle.model_oracle.OracleModel("inception", ...)``.

  * ``StepStream``      literal ring buffers, one ``step`` per frame:
                        stem i: Stream(Conv2D(k_i x 1, valid, no bias), use_one_step=True) + SSN + ReLU (inception.py:256-274);
                        the ring holds k_i rows of the layer's input INCLUDING the current frame (layers/stream.py:241-245,
                        :566-575): shift one row out, append the frame, convolve the k_i rows;
                        block: b1 / b2a / b3a 1x1 on the current frame; b2b / b3b / b3c Stream(Conv2D(k x 1, dilation d,
                        valid), use_one_step=False, pad_time_dim="None") with a ring of d(k - 1) rows of their own input
                        (stream.py:246-255): concatenate ring and input, keep the last d(k - 1) rows, convolve valid.  "None"
                        is neither causal nor same: no padding, no Delay (inception.py:121-122, stream.py:671-693);
                        StridedDrop is the identity outside NON_STREAM_INFERENCE (strided_drop.py:40-44), so the branches
                        are concatenated at the current frame and reduced by the 1x1 conv + BN + ReLU;
                        head: Stream(Flatten()) (use_one_step=True: T_f rows including the current one, stream.py:273-283),
                        Dropout inactive, Dense(1, sigmoid);
                        SSN / BN with the moving statistics, eps 1e-3, channel c -> slot c mod g
                        (sub_spectral_normalization.py:38-62); every ring starts as zeros (stream.py:580-594).
  * ``whole_sequence``  the vectorised form: every stateful layer's input left-padded with the rows that can still influence
                        an output (k_i - 1, d(k - 1), T_f - 1), every layer valid and right-aligned, the Dense at every
                        position of the final map.  The Dense is summed frame by frame of its window, so no [n, C, T_f]
                        tensor is built: hundreds of thousands of frames are fine.
  * ``non_stream_windows``  the non-streaming model (the pinned graph oracle) on the windows ending at T, T + 1, ... <= L,
                        evaluated in chunks.
``Net(..., dtype=np.float32)`` runs the same restatement in float32: its distance from the float64 form is the rounding a
float32 implementation of these sums carries (the input condition of the kernel tests).  ``StepStream.state()`` and
``whole_sequence(..., rings=True)`` give the rows that can still influence an output in the layout of
mww_stream_get_state for a graph stream: stem i [k_i - 1][C_in] (stem 0: raw input frames), per block b2b, b3b, b3c
[d(k - 1)][f1] each, the head [T_f - 1][C_last].  The reference's use_one_step=True variables (stems, head) carry one more
row each - the oldest - which is shifted out before it is read again; it is not part of the state here.
"""
from __future__ import annotations

import numpy as np

from oracle import model_oracle as mo

BN_EPS = 1e-3


class Net:
    def __init__(self, flags, om, dtype=np.float64):
        self.flags = flags
        self.dtype = np.dtype(dtype)
        self.w = {v.name: np.asarray(v.value, self.dtype) for v in om.vars}
        g = lambda n: mo.parse(flags[n])   # noqa: E731
        self.stem = [(int(k), int(gr)) for k, gr in zip(g("cnn1_kernel_sizes"), g("cnn1_subspectral_groups"))]
        self.blocks = [(int(k), int(gr), int(d)) for k, gr, d in zip(g("cnn2_kernel_sizes"), g("cnn2_subspectral_groups"), g("cnn2_dilation"))]
        self.c_last = self.w["i%d.red.kernel" % (len(self.blocks) - 1)].shape[3] if self.blocks else self.w["stem%d.kernel" % (len(self.stem) - 1)].shape[3]
        self.wd = self.w["dense.kernel"][:, 0]
        self.bd = self.w["dense.bias"][0]
        self.tf = self.wd.size // self.c_last

    def conv(self, name, groups, mem, dilation=1):
        """Conv2D(k x 1, dilation, valid, no bias) + SSN(groups) / BN + ReLU over mem [n, Cin] -> [n - d(k - 1), Cout]"""
        kern = self.w[name + ".kernel"][:, 0]   # [k, Cin, Cout]
        k, cout = kern.shape[0], kern.shape[2]
        m = mem.shape[0] - dilation * (k - 1)
        if m <= 0:
            return np.zeros((0, cout), self.dtype)
        y = np.zeros((m, cout), self.dtype)
        for j in range(k):
            y = y + mem[j * dilation:j * dilation + m] @ kern[j]
        slot = np.arange(cout) % groups if groups > 1 else np.arange(cout)
        gamma, beta = self.w[name + ".bn.gamma"][slot], self.w[name + ".bn.beta"][slot]
        mu, var = self.w[name + ".bn.moving_mean"][slot], self.w[name + ".bn.moving_variance"][slot]
        return np.maximum((y - mu) / np.sqrt(var + self.dtype.type(BN_EPS)) * gamma + beta, 0)

    def ring_shapes(self):
        """(name, rows, channels) of every ring in state order"""
        out, c = [], 40
        for i, (k, _) in enumerate(self.stem):
            out.append(("stem%d" % i, k - 1, c))
            c = self.w["stem%d.kernel" % i].shape[3]
        for i, (k, _, d) in enumerate(self.blocks):
            f1 = self.w["i%d.b2b.kernel" % i].shape[3]
            out += [("i%d.%s" % (i, b), d * (k - 1), f1) for b in ("b2b", "b3b", "b3c")]
        return out + [("head", self.tf - 1, self.c_last)]

    def n_state(self):
        return sum(r * c for _, r, c in self.ring_shapes())

    def reach(self):
        """frames in front of an output that influence it (T - 1 of the non-streaming window)"""
        return sum(k - 1 for k, _ in self.stem) + sum(2 * d * (k - 1) for k, _, d in self.blocks) + self.tf - 1


class StepStream:
    """One ``step`` per frame (the streaming interpreter's ``invoke``), literal rings."""

    def __init__(self, net: Net):
        self.net = net
        self.reset()

    def reset(self):
        n = self.net
        self.rings = {}
        for name, rows, c in n.ring_shapes():
            one_step = name.startswith("stem") or name == "head"   # use_one_step=True: the ring includes the current row
            self.rings[name] = np.zeros((rows + 1 if one_step else rows, c), n.dtype)

    def state(self):
        n = self.net
        parts = []
        for name, rows, _ in n.ring_shapes():
            r = self.rings[name]
            parts.append((r[1:] if r.shape[0] == rows + 1 else r).reshape(-1))
        return np.concatenate(parts)

    def _one_step(self, name, x):
        self.rings[name] = np.concatenate([self.rings[name][1:], x], 0)
        return self.rings[name]

    def _multi_step(self, name, x):
        mem = np.concatenate([self.rings[name], x], 0)
        self.rings[name] = mem[mem.shape[0] - self.rings[name].shape[0]:]
        return mem

    def step(self, frame):
        n = self.net
        x = np.asarray(frame, n.dtype).reshape(1, 40)
        for i, (k, g) in enumerate(n.stem):
            x = n.conv("stem%d" % i, g, self._one_step("stem%d" % i, x))
            assert x.shape[0] == 1
        for i, (k, g, d) in enumerate(n.blocks):
            p = "i%d." % i
            b1 = n.conv(p + "b1", g, x)
            b2 = n.conv(p + "b2b", g, self._multi_step(p + "b2b", n.conv(p + "b2a", g, x)), d)
            b3 = n.conv(p + "b3b", g, self._multi_step(p + "b3b", n.conv(p + "b3a", g, x)), d)
            b3 = n.conv(p + "b3c", g, self._multi_step(p + "b3c", b3), d)
            assert b1.shape[0] == b2.shape[0] == b3.shape[0] == 1
            x = n.conv(p + "red", 1, np.concatenate([b1, b2, b3], 1))
        return self._one_step("head", x).reshape(-1) @ n.wd + n.bd

    def run(self, frames):
        return np.array([self.step(f) for f in frames], self.net.dtype).reshape(-1)


def whole_sequence(net: Net, frames, rings=False):
    """Vectorised streaming form from zero state over ``frames`` [N, 40] -> logits [N]; with ``rings`` also the state after
    those frames."""
    dt = net.dtype
    x = np.asarray(frames, dt).reshape(-1, 40)
    N = x.shape[0]
    st = []

    def padded(a, rows):
        a = np.concatenate([np.zeros((rows, a.shape[1]), dt), a], 0)
        st.append(a[a.shape[0] - rows:].reshape(-1))
        return a

    for i, (k, g) in enumerate(net.stem):
        x = net.conv("stem%d" % i, g, padded(x, k - 1))
    for i, (k, g, d) in enumerate(net.blocks):
        p, R = "i%d." % i, d * (k - 1)
        b1 = net.conv(p + "b1", g, x)
        b2 = net.conv(p + "b2b", g, padded(net.conv(p + "b2a", g, x), R), d)
        b3 = net.conv(p + "b3b", g, padded(net.conv(p + "b3a", g, x), R), d)
        b3 = net.conv(p + "b3c", g, padded(b3, R), d)
        x = net.conv(p + "red", 1, np.concatenate([b1, b2, b3], 1))
    h = padded(x, net.tf - 1)
    W = net.wd.reshape(net.tf, -1)
    z = np.full(N, net.bd, dt)
    for t in range(net.tf):
        z = z + h[t:t + N] @ W[t]
    return (z, np.concatenate(st)) if rings else z


def non_stream_windows(om, frames, T, chunk=2048):
    """the non-streaming model on frames [e - T, e), e = T, T + 1, ... <= L -> float64 logits, ``chunk`` windows at a time"""
    frames = np.asarray(frames, np.float64)
    L = len(frames)
    if L < T:
        return np.zeros(0)
    win = np.lib.stride_tricks.sliding_window_view(frames, T, axis=0)   # [L - T + 1, 40, T] view
    out = []
    for a in range(0, win.shape[0], chunk):
        out.append(om.predict_with_logits(np.ascontiguousarray(win[a:a + chunk].transpose(0, 2, 1)))[1].reshape(-1))
    return np.concatenate(out)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))
