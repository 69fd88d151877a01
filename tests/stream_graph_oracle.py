"""TEST INFRASTRUCTURE: float64 restatement of the streaming conv -> BN/SSN -> ReLU graph of ``native.GraphStream``
(csrc/tu_stream_graph.hip), driven by the description dict the stream takes (``conv_ops`` with src / drop / slice / kernel /
dilation / filters / bn_groups; ``frames``; ``mode``) and its Keras-order weights (per op kernel [k,1,Cin,F], gamma, beta,
moving mean, moving variance [slots]; dense kernel [T_f * C, 1], bias) - any DAG the planner accepts, not only an Inception
(tests/inception_streaming_oracle.py is driven by Inception flags).  Written apart from the kernel, after
tests/quant_graph_oracle.py: BN / SSN folded in float64 (moving statistics, eps 1e-3, channel c in slot c mod g), rings literal.

  * ``StepStream``          one ``step`` per frame: every op with R = d(k - 1) > 0 keeps a ring of R rows of its concatenated
                            input (all sources' slices side by side), the head T_f - 1 rows of the final map; rings start as
                            zeros.
  * ``whole_sequence``      the vectorised form: each such op's input left-padded with its ring, every op valid and
                            right-aligned, the Dense at every position -> logits (and the flat state in the layout of
                            mww_stream_get_state: per op with R > 0 [R][Cin], then the head [T_f - 1][C_last]).
  * ``non_stream_windows``  the windows ending at frames T, T + 1, ...: no ring anywhere; the ops are applied to each window,
                            ``drop`` removing leading frames of a source (StridedDrop).
  * ``Net(..., dtype=np.float32)``  the same sums in float32 with the weights folded in float64 and rounded to float32, as a
                            float32 implementation holds them: its distance from the float64 form is the rounding such an
                            implementation carries (the input condition of the kernel tests).
``Net(..., without=(op, source))`` / ``without=(op, None, tap)`` restate the graph with one source or one tap of one op
zeroed: what a kernel that lost that source or tap would compute (the sensitivity condition of tests/stream_graph_sweep.py).
"""
from __future__ import annotations

import numpy as np

BN_EPS = 1e-3
BINS = 40


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


class Net:
    def __init__(self, desc, weights, dtype=np.float64, without=None):
        self.dtype = np.dtype(dtype)
        self.ops = []
        ch = [BINS]
        it = iter(weights)
        for i, o in enumerate(desc["conv_ops"]):
            src = [int(s) for s in o["src"]]
            drop = [int(v) for v in o.get("drop", [0] * len(src))]
            sl = [(int(a), int(b)) for a, b in o.get("slice", [(0, 0)] * len(src))]
            parts = [(s + 1, c0, cn if cn else ch[s + 1] - c0, dr) for s, (c0, cn), dr in zip(src, sl, drop)]
            k, d, co, g = int(o["kernel"]), int(o.get("dilation", 1)), int(o["filters"]), int(o.get("bn_groups", 1))
            cin = sum(p[2] for p in parts)
            kern, gamma, beta, mean, var = (np.asarray(next(it), np.float64) for _ in range(5))
            slot = np.arange(co) % g if g > 1 else np.arange(co)
            sc = gamma[slot] / np.sqrt(var[slot] + BN_EPS)
            w = kern.reshape(k, cin, co) * sc[None, None, :]
            b = beta[slot] - mean[slot] * sc
            if self.dtype != np.float64:   # the folded values a float32 implementation holds
                w, b = w.astype(np.float32), b.astype(np.float32)
            if without is not None and without[0] == i:
                w = w.copy()
                if without[1] is not None:
                    at = sum(p[2] for p in parts[:without[1]])
                    w[:, at:at + parts[without[1]][2]] = 0
                else:
                    w[without[2]] = 0
            self.ops.append(dict(parts=parts, k=k, d=d, R=d * (k - 1), cin=cin, co=co, w=w.astype(self.dtype), b=b.astype(self.dtype)))
            ch.append(co)
        self.n = len(self.ops)
        self.c_last = ch[-1]
        wd = np.asarray(next(it), np.float64).reshape(-1)
        self.bd = self.dtype.type(np.asarray(next(it), np.float64).reshape(-1)[0])
        assert next(it, None) is None and wd.size % self.c_last == 0
        self.tf = wd.size // self.c_last
        self.wd = wd.reshape(self.tf, self.c_last).astype(self.dtype)

    def gather(self, i, tensors, drop=False):
        """the concatenated input of op i: its sources' slices side by side, right-aligned (stream mode: every tensor has
        one row per frame) or with each source's leading ``drop`` rows removed (non-stream mode)"""
        parts = [tensors[t][..., (dr if drop else 0):, c0:c0 + cn] for t, c0, cn, dr in self.ops[i]["parts"]]
        m = min(p.shape[-2] for p in parts)
        assert not drop or all(p.shape[-2] == m for p in parts), "drop does not align the sources"
        return np.concatenate([p[..., p.shape[-2] - m:, :] for p in parts], -1)

    def conv(self, i, mem):
        """op i valid over mem [..., n, Cin] -> [..., n - R, Co]: taps, folded BN / SSN, ReLU"""
        op = self.ops[i]
        m = mem.shape[-2] - op["R"]
        assert m > 0
        y = np.zeros(mem.shape[:-2] + (m, op["co"]), self.dtype) + op["b"]
        for j in range(op["k"]):
            y = y + mem[..., j * op["d"]:j * op["d"] + m, :] @ op["w"][j]
        return np.maximum(y, 0)

    def head(self, h):
        """Dense at every position of h [n + T_f - 1, C] -> [n]"""
        n = h.shape[0] - self.tf + 1
        z = np.full(n, self.bd, self.dtype)
        for t in range(self.tf):
            z = z + h[t:t + n] @ self.wd[t]
        return z

    def ring_shapes(self):
        """(op or "head", rows, channels, fed by the spectrogram alone) of every ring in state order"""
        out = [(i, op["R"], op["cin"], all(p[0] == 0 for p in op["parts"])) for i, op in enumerate(self.ops) if op["R"]]
        return out + ([("head", self.tf - 1, self.c_last, False)] if self.tf > 1 else [])

    def n_state(self):
        return sum(r * c for _, r, c, _ in self.ring_shapes())


class StepStream:
    """one ``step`` per frame, literal rings"""

    def __init__(self, net: Net):
        self.net = net
        self.reset()

    def reset(self):
        n = self.net
        self.rings = {i: np.zeros((op["R"], op["cin"]), n.dtype) for i, op in enumerate(n.ops) if op["R"]}
        self.hring = np.zeros((n.tf - 1, n.c_last), n.dtype)

    def state(self):
        return np.concatenate([self.rings[i].reshape(-1) for i in sorted(self.rings)] + [self.hring.reshape(-1)])

    def step(self, frame):
        n = self.net
        tensors = [np.asarray(frame, n.dtype).reshape(1, BINS)]
        for i, op in enumerate(n.ops):
            x = n.gather(i, tensors)
            if op["R"]:
                x = np.concatenate([self.rings[i], x], 0)
                self.rings[i] = x[1:]
            tensors.append(n.conv(i, x))
            assert tensors[-1].shape[0] == 1
        h = np.concatenate([self.hring, tensors[-1]], 0)
        self.hring = h[1:]
        return n.head(h)[0]

    def run(self, frames):
        return np.array([self.step(f) for f in np.asarray(frames).reshape(-1, BINS)], self.net.dtype).reshape(-1)


def whole_sequence(net: Net, frames, rings=False, tensors_out=None):
    """from zero state over ``frames`` [N, 40] -> logits [N]; with ``rings`` also the state after those frames.
    ``tensors_out``: a list that receives every tensor (the input, every op's output)."""
    x = np.asarray(frames, net.dtype).reshape(-1, BINS)
    tensors, st = [x], []
    for i, op in enumerate(net.ops):
        a = net.gather(i, tensors)
        if op["R"]:
            a = np.concatenate([np.zeros((op["R"], op["cin"]), net.dtype), a], 0)
            st.append(a[a.shape[0] - op["R"]:].reshape(-1))
        tensors.append(net.conv(i, a) if x.shape[0] else np.zeros((0, op["co"]), net.dtype))
    h = np.concatenate([np.zeros((net.tf - 1, net.c_last), net.dtype), tensors[-1]], 0)
    st.append(h[h.shape[0] - (net.tf - 1):].reshape(-1))
    z = net.head(h)
    if tensors_out is not None:
        tensors_out[:] = tensors
    return (z, np.concatenate(st)) if rings else z


def non_stream_windows(net: Net, frames, T, chunk=64):
    """the non-streaming model on frames [e - T, e), e = T, T + 1, ... <= L -> logits, ``chunk`` windows at a time; every
    window is run on its own (batched), ``drop`` aligning the sources of an op"""
    frames = np.asarray(frames, net.dtype).reshape(-1, BINS)
    L = len(frames)
    if L < T:
        return np.zeros(0, net.dtype)
    win = np.lib.stride_tricks.sliding_window_view(frames, T, axis=0)   # [L - T + 1, 40, T] view
    out = []
    for a in range(0, win.shape[0], chunk):
        tensors = [np.ascontiguousarray(win[a:a + chunk].transpose(0, 2, 1))]
        for i in range(net.n):
            tensors.append(net.conv(i, net.gather(i, tensors, drop=True)))
        f = tensors[-1]
        assert f.shape[1] == net.tf, "the window does not leave T_f final frames"
        out.append(np.einsum("wtc,tc->w", f, net.wd) + net.bd)
    return np.concatenate(out)
