"""What the model is, on the host: flag parsing, shape derivation and the Keras-order <-> native-order weight mapping of
MixedNet and Inception.  Two facts are stated once here and consumed everywhere else:

  * ``MixedNetTopology``   the ONE walk over a MixedNet flag set: the per-block lists, the first convolution, every layer
                           with its channels and frame counts, T_f and the head options.  ``MixedNetLayout`` and
                           ``GraphMixedNetLayout`` below, ``streaming.stream_description`` /
                           ``streaming.mixednet_stream_description`` and (through ``mixednet_layers``) ``quantize.plan_ops``
                           consume it; each keeps only its own refusals.
  * ``NativeWeights``      the ONE mapping between ``get_weights()`` and the native parameter / state vectors, derived from
                           a layout's ``table`` of pieces: ``Concat`` (Keras variables concatenated along the last axis) and
                           ``MixConv`` (the groups of a MixConv fused to one depthwise).  The three layouts fill the table;
                           ``pack`` / ``unpack`` / ``segments`` / ``grad_mask`` / the counts exist once.
                           ``quantize.fold_mixconv`` fuses with the same ``mixconv_fuse``.

Mirrors the host-side arithmetic of the reference (no tensors involved):
  * ``parse``                         microwakeword/mixednet.py:25-40
  * ``spectrogram_slices_dropped``    microwakeword/mixednet.py:108-129
  * list-length check / ValueError    microwakeword/mixednet.py:298-305
  * ``_split_channels``               microwakeword/mixednet.py:132-136
  * layer creation order (= Keras ``get_weights()`` order)  microwakeword/mixednet.py:307-386, SURVEY §A.4

Native order (``include/mww.h``): trainable scalars in Keras order with every multi-kernel
MixConv fused into one ``[K_last, C]`` depthwise whose missing leading taps are structural zeros
(mixednet.py:218-230 + strided_drop.py:42 => right alignment), plus a 0/1 gradient mask; BN moving
statistics live in a separate state vector.
"""
from __future__ import annotations

import ast
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

FEATURE_BINS = 40


def parse(text):
    if not text:
        return []
    res = ast.literal_eval(text) if isinstance(text, str) else text
    if isinstance(res, tuple):
        return res
    if isinstance(res, list):
        return tuple(res)
    return [res]


def _flag(flags, name):
    return flags[name] if isinstance(flags, dict) else getattr(flags, name)


def split_channels(total_filters, num_groups):
    split = [total_filters // num_groups for _ in range(num_groups)]
    split[0] += total_filters - sum(split)
    return split


def spectrogram_slices_dropped(flags) -> int:
    dropped = 0
    if _flag(flags, "first_conv_filters") > 0:
        dropped += _flag(flags, "first_conv_kernel_size") - 1
    for repeat, ksize in zip(parse(_flag(flags, "repeat_in_block")), parse(_flag(flags, "mixconv_kernel_sizes"))):
        dropped += (repeat * (max(ksize) - 1)) * _flag(flags, "stride")
    return dropped


def _too_short(frames):
    return ValueError("spectrogram of %d frames is too short for this network" % frames)


# ------------------------------------------------------------------------------------------------ MixConv, fused
def _mixconv_slots(groups):
    """per group (channels, k) of one MixConv its (rows, columns) in the fused [K, C] tap table, K the largest k: the taps are
    right-aligned (mixednet.py:218-230 + strided_drop.py:42), the rows above them structural zeros"""
    K, c0 = max(k for _, k in groups), 0
    for gc, k in groups:
        yield slice(K - k, K), slice(c0, c0 + gc)
        c0 += gc


def mixconv_fuse(groups, arrays):
    """the groups (channels, k) of one MixConv, each taking its kernel [k,1,gc,1] and bias [gc] from the iterator ``arrays``
    -> the depthwise tap table [K, C] and bias [C]"""
    K, C = max(k for _, k in groups), sum(gc for gc, _ in groups)
    dw, bias = np.zeros((K, C), np.float32), np.zeros(C, np.float32)
    for (gc, k), (rows, cols) in zip(groups, _mixconv_slots(groups)):
        dw[rows, cols] = next(arrays).reshape(k, gc)
        bias[cols] = next(arrays).reshape(gc)
    return dw, bias


def mixconv_split(groups, dw, bias):
    """``mixconv_fuse`` backwards: [kernel [k,1,gc,1], bias [gc]] of every group, copies"""
    out = []
    for (gc, k), (rows, cols) in zip(groups, _mixconv_slots(groups)):
        out += [dw[rows, cols].reshape(k, 1, gc, 1).copy(), bias[cols].copy()]
    return out


def mixconv_mask(groups):
    """0/1 [K, C]: 0 on the structural zeros of the fused tap table"""
    m = np.zeros((max(k for _, k in groups), sum(gc for gc, _ in groups)), np.float32)
    for rows, cols in _mixconv_slots(groups):
        m[rows, cols] = 1.0
    return m


# --------------------------------------------------------------------------------- Keras order <-> native order
def _size(shape):
    return int(np.prod(shape))


class Concat:
    """native piece: the Keras variables ``idxs`` concatenated along the last axis (one variable: the variable itself)"""

    def __init__(self, name, kind, idxs):
        self.name, self.kind, self.idxs = name, kind, list(idxs)

    def segments(self, kv):
        return [(self.name, sum(_size(kv[i][1]) for i in self.idxs))]

    def pack(self, ws):
        v = ws[self.idxs[0]] if len(self.idxs) == 1 else np.concatenate([ws[i] for i in self.idxs], axis=-1)
        return v.reshape(-1)

    def unpack(self, flat, kv, out):
        shapes = [kv[i][1] for i in self.idxs]
        merged = flat.reshape(shapes[0][:-1] + (sum(sh[-1] for sh in shapes),))
        c0 = 0
        for i, sh in zip(self.idxs, shapes):
            out[i] = merged[..., c0:c0 + sh[-1]].copy()
            c0 += sh[-1]

    def mask(self, kv):
        return np.ones(self.segments(kv)[0][1], np.float32)


class MixConv:
    """native piece: one MixConv's ``groups`` (index of the group's kernel in keras_vars - its bias follows -, channels, k)
    as the fused tap table ``name.kernel`` [K, C] and ``name.bias`` [C]"""
    kind = "param"

    def __init__(self, name, groups):
        self.name, self.groups = name, list(groups)
        self.parts = [(gc, k) for _, gc, k in self.groups]   # (channels, k)
        self.K, self.C = max(k for _, k in self.parts), sum(gc for gc, _ in self.parts)

    def segments(self, kv):
        return [(self.name + ".kernel", self.K * self.C), (self.name + ".bias", self.C)]

    def pack(self, ws):
        dw, bias = mixconv_fuse(self.parts, (ws[vi + j] for vi, _, _ in self.groups for j in (0, 1)))
        return np.concatenate([dw.reshape(-1), bias])

    def unpack(self, flat, kv, out):
        arrays = mixconv_split(self.parts, flat[:self.K * self.C].reshape(self.K, self.C), flat[self.K * self.C:])
        for g, (vi, _, _) in enumerate(self.groups):
            out[vi], out[vi + 1] = arrays[2 * g], arrays[2 * g + 1]

    def mask(self, kv):
        return np.concatenate([mixconv_mask(self.parts).reshape(-1), np.ones(self.C, np.float32)])


class NativeWeights:
    """What every layout derives from its ``keras_vars`` [(name, shape, "param" | "state")] (``get_weights()`` order) and its
    ``table``, the native pieces in native order (``Concat`` / ``MixConv``, each "param" or "state"): the parameter pieces in
    order are the native parameter vector, the state pieces the BN state vector."""

    keras_vars: List[Tuple[str, Tuple[int, ...], str]]
    table: list

    def _var(self, name, shape, kind="param", piece=None):
        """a Keras variable that is a native piece of its own (named ``piece`` where the op's name is not the variable's)"""
        self.keras_vars.append((name, tuple(int(n) for n in shape), kind))
        self.table.append(Concat(piece or name, kind, [len(self.keras_vars) - 1]))

    def _bn(self, prefix, channels, piece=None):
        for suffix, kind in (("gamma", "param"), ("beta", "param"), ("moving_mean", "state"), ("moving_variance", "state")):
            self._var("%s.bn.%s" % (prefix, suffix), (channels,), kind, "%s.bn.%s" % (piece or prefix, suffix))

    def _mixconv(self, prefix, piece, channels, kernel_sizes):
        """the variables of one MixConv over ``channels`` (``prefix.dw<g>.kernel`` / ``.bias`` per group) and its fused piece"""
        groups = []
        for gi, (gc, k) in enumerate(zip(split_channels(channels, len(kernel_sizes)), kernel_sizes)):
            groups.append((len(self.keras_vars), int(gc), int(k)))
            self.keras_vars.append(("%s.dw%d.kernel" % (prefix, gi), (int(k), 1, int(gc), 1), "param"))
            self.keras_vars.append(("%s.dw%d.bias" % (prefix, gi), (int(gc),), "param"))
        self.table.append(MixConv(piece, groups))
        return self.table[-1]

    def _count(self, kind):
        return sum(n for p in self.table if p.kind == kind for _, n in p.segments(self.keras_vars))

    @property
    def n_params(self):
        return self._count("param")

    @property
    def n_state(self):
        return self._count("state")

    def keras_param_counts(self):
        """(total, trainable) as Keras would report them"""
        return sum(_size(s) for _, s, _ in self.keras_vars), sum(_size(s) for _, s, kind in self.keras_vars if kind == "param")

    def segments(self):
        """(name, size) of every contiguous piece of the native parameter vector, in order."""
        return [seg for p in self.table if p.kind == "param" for seg in p.segments(self.keras_vars)]

    def grad_mask(self) -> np.ndarray:
        return np.concatenate([p.mask(self.keras_vars) for p in self.table if p.kind == "param"])

    def pack(self, weights: Sequence[np.ndarray]):
        """Keras list -> native (parameter vector, state vector)"""
        if len(weights) != len(self.keras_vars):
            raise ValueError("expected %d weight arrays, got %d" % (len(self.keras_vars), len(weights)))
        ws = []
        for (name, shape, _), w in zip(self.keras_vars, weights):
            w = np.asarray(w, np.float32)
            if tuple(w.shape) != tuple(shape):
                raise ValueError("weight %s: expected shape %s, got %s" % (name, shape, w.shape))
            ws.append(w)
        vec = {kind: [p.pack(ws) for p in self.table if p.kind == kind] for kind in ("param", "state")}
        return np.concatenate(vec["param"]), (np.concatenate(vec["state"]) if vec["state"] else np.zeros(0, np.float32))

    def unpack(self, params: np.ndarray, state: np.ndarray) -> List[np.ndarray]:
        at = {"param": [np.asarray(params, np.float32).reshape(-1), 0], "state": [np.asarray(state, np.float32).reshape(-1), 0]}
        if at["param"][0].size != self.n_params or at["state"][0].size != self.n_state:
            raise ValueError("vector sizes do not match this model")
        out: List[Optional[np.ndarray]] = [None] * len(self.keras_vars)
        for p in self.table:
            vec, o = at[p.kind]
            n = sum(n for _, n in p.segments(self.keras_vars))
            p.unpack(vec[o:o + n], self.keras_vars, out)
            at[p.kind][1] = o + n
        return out


# ------------------------------------------------------------------------------------------------ MixedNet topology
def mixednet_layers(channels, blocks, residual):
    """The layers behind a MixedNet's first convolution (mixednet.py:307-360), ``channels`` wide at their input, of ``blocks``
    [(repeat, kernel sizes, filters)] with ``residual`` flags: [(kind, block, repeat, kernel sizes, cin, cout)], kind "res" (a
    block's residual 1x1, repeat None), "mix" (MixConv, only when its largest kernel exceeds 1), "pw" (1x1 + ReLU) or
    "pw_add" (linear 1x1, then ADD + ReLU)."""
    out, c = [], channels
    for b, ((rep, ks, f), res) in enumerate(zip(blocks, residual)):
        if res:
            out.append(("res", b, None, ks, c, f))
        for r in range(rep):
            if max(ks) > 1:
                out.append(("mix", b, r, ks, c, c))
            out.append(("pw_add" if res else "pw", b, r, ks, c, f))
            c = f
    return out


def block_lists(flags):
    """the per-block lists of a MixedNet flag set: pointwise filters, repeats, kernel-size tuples, residual flags (as given)"""
    pf = [int(f) for f in parse(_flag(flags, "pointwise_filters"))]
    rep = [int(r) for r in parse(_flag(flags, "repeat_in_block"))]
    ksz = [tuple(int(k) for k in (ks if isinstance(ks, (list, tuple)) else (ks,))) for ks in parse(_flag(flags, "mixconv_kernel_sizes"))]
    res = list(parse(_flag(flags, "residual_connection")))
    for lst in (rep, ksz, res):
        if len(pf) != len(lst):
            raise ValueError("all input lists have to be the same length")  # mixednet.py:298-305
    return pf, rep, ksz, res


@dataclass
class Layer:
    kind: str                        # "conv1", or a kind of ``mixednet_layers``
    block: Optional[int]
    repeat: Optional[int]
    kernel_sizes: Tuple[int, ...]
    cin: int
    cout: int
    tin: int
    tout: int


class MixedNetTopology:
    """The walk over a MixedNet flag set and ``frames`` input frames (mixednet.py:307-386).  ``filters`` / ``repeats`` /
    ``kernels`` / ``residual``: the per-block lists (ValueError when their lengths differ); ``conv1``: the first convolution's
    ``Layer`` or None without one; ``blocks``: per block the ``Layer``s of ``mixednet_layers`` with their frame counts (a
    MixConv drops max(ks) - 1 frames, a residual 1x1 none); ``t_final`` / ``c_final``: the final map BEFORE the head options.
    It only does the arithmetic: a frame count may come out <= 0, and what is refused (too few frames, kernel sizes that do
    not ascend, a missing first convolution, ...) is each consumer's own decision, in its own order."""

    def __init__(self, flags, frames: int):
        self.filters, self.repeats, self.kernels, self.residual = block_lists(flags)
        self.frames = int(frames)
        self.conv1_filters = int(_flag(flags, "first_conv_filters"))
        self.conv1_kernel = int(_flag(flags, "first_conv_kernel_size"))
        self.stride = int(_flag(flags, "stride"))
        self._attention = bool(_flag(flags, "spatial_attention"))
        self._pool = (2 if _flag(flags, "max_pool") else 1) if _flag(flags, "pooled") else 0
        t, c = self.frames, FEATURE_BINS
        self.conv1 = None
        if self.conv1_filters > 0:
            self.conv1 = Layer("conv1", None, None, (self.conv1_kernel,), c, self.conv1_filters, t, (t - self.conv1_kernel) // self.stride + 1)
            t, c = self.conv1.tout, self.conv1_filters
        self.blocks: List[List[Layer]] = [[] for _ in self.filters]
        for kind, b, r, ks, cin, cout in mixednet_layers(c, zip(self.repeats, self.kernels, self.filters), self.residual):
            tout = t - (max(ks) - 1) if kind == "mix" else t
            self.blocks[b].append(Layer(kind, b, r, ks, cin, cout, t, tout))
            if kind != "res":
                t, c = tout, cout
        self.t_final, self.c_final = t, c

    def head(self):
        """(spatial attention, pooling 0 / 1 average / 2 max, frames the Dense reads): with one frame left the head options do
        nothing (mixednet.py:362); ValueError when SpatialAttention(kernel_size=4) has fewer than four frames"""
        if self.t_final <= 1:
            return False, 0, self.t_final
        if self._attention and self.t_final < 4:
            raise ValueError("spatial attention needs at least 4 frames after the last block")
        t = self.t_final - 3 if self._attention else self.t_final
        return self._attention, self._pool, 1 if self._pool else t


@dataclass
class BlockSpec:
    cin: int
    cout: int
    kernel_sizes: Tuple[int, ...]
    group_channels: Tuple[int, ...]
    tin: int
    tout: int

    @property
    def k(self):
        return self.kernel_sizes[-1]


def _ascending(ks):
    if any(k > ks[-1] for k in ks):
        raise ValueError("mixconv kernel sizes must be ascending: alignment uses the last one (mixednet.py:227)")


class MixedNetLayout(NativeWeights):
    """The MixedNets the specialised block kernels cover: a first convolution, then per block one MixConv (a depthwise
    convolution, kernel size above 1) and one 1x1 + BN + ReLU; a flattening Dense."""

    def __init__(self, flags, frames: int):
        topo = MixedNetTopology(flags, frames)
        self.frames = topo.frames
        self.conv1_filters, self.conv1_kernel, self.stride = topo.conv1_filters, topo.conv1_kernel, topo.stride
        unsupported = []
        if self.conv1_filters <= 0:
            unsupported.append("first_conv_filters == 0")
        if any(topo.residual):
            unsupported.append("residual_connection")
        if any(r != 1 for r in topo.repeats):
            unsupported.append("repeat_in_block != 1")
        if _flag(flags, "spatial_attention"):
            unsupported.append("spatial_attention")
        if _flag(flags, "pooled"):
            unsupported.append("pooled")
        if unsupported:
            raise NotImplementedError("MixedNet options outside the specialised block kernels (GraphMixedNetLayout covers them): "
                                      + ", ".join(unsupported))
        self.keras_vars, self.table = [], []
        self._var("conv1.kernel", (self.conv1_kernel, 1, FEATURE_BINS, self.conv1_filters))
        self.blocks: List[BlockSpec] = []
        for bi, (ks, layers) in enumerate(zip(topo.kernels, topo.blocks)):
            if max(ks) <= 1:
                raise NotImplementedError("blocks without a depthwise convolution (kernel size 1)")
            _ascending(ks)
            mix, pw = layers
            if mix.tout <= 0:
                raise _too_short(frames)
            groups = self._mixconv("b%d" % bi, "b%d.dw" % bi, mix.cin, ks).parts
            self.blocks.append(BlockSpec(mix.cin, pw.cout, ks, tuple(gc for gc, _ in groups), mix.tin, mix.tout))
            self._var("b%d.pw.kernel" % bi, (1, 1, pw.cin, pw.cout))
            self._bn("b%d" % bi, pw.cout)
        self.t_last, self.c_last = topo.t_final, topo.c_final
        self._var("dense.kernel", (self.t_last * self.c_last, 1))
        self._var("dense.bias", (1,))

    def engine_args(self, max_batch):
        return dict(frames=self.frames, conv1_filters=self.conv1_filters, conv1_kernel=self.conv1_kernel,
                    conv1_stride=self.stride, block_filters=[b.cout for b in self.blocks],
                    block_kernel=[b.k for b in self.blocks], max_batch=max_batch)

    def summary_lines(self):
        yield "input                      [B, %d, %d]" % (self.frames, FEATURE_BINS)
        yield "conv1 %dx1 /%d -> %d, relu    [B, %d, %d]" % (self.conv1_kernel, self.stride, self.conv1_filters, self.blocks[0].tin, self.conv1_filters)
        for i, b in enumerate(self.blocks):
            yield "block %d: mixconv %s + 1x1 %d->%d + BN + relu   [B, %d, %d]" % (i, list(b.kernel_sizes), b.cin, b.cout, b.tout, b.cout)
        yield "flatten + dense(1, sigmoid)  [B, 1]"


class InceptionLayout(NativeWeights):
    """Shape derivation and Keras-order weight mapping of the reference's Inception model
    (microwakeword/inception.py:232-340) as a list of conv -> BN/SSN -> ReLU ops for
    ``mww_create_convnet`` (include/mww.h).

      * stem: Conv2D(k x 1, valid, no bias) + SubSpectralNormalization + ReLU   inception.py:261-279
      * block: branch1 1x1; branch2 1x1 -> kx1; branch3 1x1 -> kx1 -> kx1; StridedDrop of the leading
        frames of branch1/2 to branch3's length; concatenate; 1x1 reduce         inception.py:281-328
      * Flatten -> Dropout -> Dense(1, sigmoid)                                  inception.py:330-338
      * ``spectrogram_slices_dropped``                                           inception.py:212-230

    ``keras_vars`` is ``get_weights()`` order (layer-creation order).  The native order differs in one
    place: with plain BatchNormalization (sub-spectral groups == 1) the three 1x1 branch heads of a block
    read the same input, so they run as ONE convolution with the concatenated filters (``fuse_heads``);
    its kernel / gamma / beta / moving statistics are the three layers' arrays concatenated along the
    channel axis (a ``Concat`` piece of three variables), and each consumer names its channel slice.
    """

    def __init__(self, flags, frames: int, fuse_heads: bool = True):
        self.frames = int(frames)
        self.dropout = float(_flag(flags, "dropout"))
        stem = list(zip(parse(_flag(flags, "cnn1_filters")), parse(_flag(flags, "cnn1_kernel_sizes")),
                        parse(_flag(flags, "cnn1_subspectral_groups"))))
        blocks = list(zip(parse(_flag(flags, "cnn2_filters1")), parse(_flag(flags, "cnn2_filters2")),
                          parse(_flag(flags, "cnn2_kernel_sizes")), parse(_flag(flags, "cnn2_subspectral_groups")),
                          parse(_flag(flags, "cnn2_dilation"))))
        self.ops: List[dict] = []
        self.op_names: List[str] = []
        self.op_members: List[List[Tuple[str, int, int]]] = []   # per native op: (keras layer name, first channel, width)
        self.keras_vars, self.table = [], []
        kidx = {}   # keras layer name -> index of its kernel in keras_vars (gamma +1, beta +2, mean +3, var +4)
        t, c = self.frames, FEATURE_BINS
        cur = (-1, 0, 0)   # (op index, first channel, width) of the running tensor; width 0 = whole

        def keras_layer(name, k, cin, filters, groups):
            if filters % groups:
                # sub_spectral_normalization.py:41-45
                raise ValueError("input_shape[3]: %d must be divisible by self.sub_groups %d " % (filters, groups))
            slots = groups if groups > 1 else filters
            kidx[name] = len(self.keras_vars)
            self.keras_vars.append((name + ".kernel", (int(k), 1, int(cin), int(filters)), "param"))
            self.keras_vars.append((name + ".bn.gamma", (slots,), "param"))
            self.keras_vars.append((name + ".bn.beta", (slots,), "param"))
            self.keras_vars.append((name + ".bn.moving_mean", (slots,), "state"))
            self.keras_vars.append((name + ".bn.moving_variance", (slots,), "state"))

        def add(names, srcs, cin, tin, k, dil, filters_each, groups):
            """one native op computing the Keras layers ``names`` (same input, same shape) side by side"""
            tout = tin - (k - 1) * dil
            if tout <= 0:
                raise _too_short(frames)
            filters = filters_each * len(names)
            self.ops.append(dict(src=[s[0] for s in srcs], drop=[s[3] for s in srcs], slice=[(s[1], s[2]) for s in srcs],
                                 kernel=int(k), dilation=int(dil), filters=int(filters), bn_groups=int(groups), cin=int(cin),
                                 tin=int(tin), tout=int(tout), slots=int(groups if groups > 1 else filters)))
            self.op_names.append("+".join(names))
            self.op_members.append([(n, i * filters_each, filters_each) for i, n in enumerate(names)])
            return len(self.ops) - 1, tout

        for i, (f, k, g) in enumerate(stem):
            keras_layer("stem%d" % i, k, c, f, g)
            oi, t = add(["stem%d" % i], [cur + (0,)], c, t, k, 1, f, g)
            cur, c = (oi, 0, 0), int(f)
        for i, (f1, f2, k, g, dil) in enumerate(blocks):
            n = "i%d." % i
            for nm, kk, ci in (("b1", 1, c), ("b2a", 1, c), ("b2b", k, f1), ("b3a", 1, c), ("b3b", k, f1), ("b3c", k, f1)):
                keras_layer(n + nm, kk, ci, f1, g)
            keras_layer(n + "red", 1, 3 * f1, f2, 1)
            if fuse_heads and g == 1:
                heads, _ = add([n + "b1", n + "b2a", n + "b3a"], [cur + (0,)], c, t, 1, 1, f1, 1)
                b1, b2a, b3a = (heads, 0, f1), (heads, f1, f1), (heads, 2 * f1, f1)
            else:
                b1 = (add([n + "b1"], [cur + (0,)], c, t, 1, 1, f1, g)[0], 0, 0)
                b2a = (add([n + "b2a"], [cur + (0,)], c, t, 1, 1, f1, g)[0], 0, 0)
                b3a = (add([n + "b3a"], [cur + (0,)], c, t, 1, 1, f1, g)[0], 0, 0)
            b2, t2 = add([n + "b2b"], [b2a + (0,)], f1, t, k, dil, f1, g)
            b3b, t3b = add([n + "b3b"], [b3a + (0,)], f1, t, k, dil, f1, g)
            b3, t3 = add([n + "b3c"], [(b3b, 0, 0, 0)], f1, t3b, k, dil, f1, g)
            red, t = add([n + "red"], [b1 + (t - t3,), (b2, 0, 0, t2 - t3), (b3, 0, 0, 0)], 3 * f1, t3, 1, 1, f2, 1)
            cur, c = (red, 0, 0), int(f2)
        if not self.ops:
            raise NotImplementedError("an Inception model without any convolution")
        self.t_last, self.c_last = t, c
        for name, members in zip(self.op_names, self.op_members):   # a native op's pieces: its Keras layers' variables side by side
            base = [kidx[m[0]] for m in members]
            for off, suffix, kind in ((0, ".kernel", "param"), (1, ".bn.gamma", "param"), (2, ".bn.beta", "param"),
                                      (3, ".bn.moving_mean", "state"), (4, ".bn.moving_variance", "state")):
                self.table.append(Concat(name + suffix, kind, [b + off for b in base]))
        self._var("dense.kernel", (t * c, 1))
        self._var("dense.bias", (1,))
        # per native op: index in keras_vars of the kernel of its first Keras layer (its place in layer-creation order)
        self.op_keras_index = [kidx[members[0][0]] for members in self.op_members]

    def engine_args(self, max_batch):
        return dict(frames=self.frames, conv_ops=self.ops, dropout=self.dropout, max_batch=max_batch)

    def summary_lines(self):
        yield "input                                   [B, %d, %d]" % (self.frames, FEATURE_BINS)
        for name, op in zip(self.op_names, self.ops):
            norm = "SSN(%d)" % op["bn_groups"] if op["bn_groups"] > 1 else "BN"
            yield "%-22s conv %dx1 d%d %d->%d + %s + relu   [B, %d, %d]" % (name, op["kernel"], op["dilation"], op["cin"], op["filters"],
                                                                           norm, op["tout"], op["filters"])
        yield "flatten + dropout(%g) + dense(1, sigmoid)   [B, 1]" % self.dropout


def inception_slices_dropped(flags) -> int:
    """inception.py:212-230."""
    dropped = 0
    for kernel_size in parse(_flag(flags, "cnn1_kernel_sizes")):
        dropped += kernel_size - 1
    for kernel_size, dilation in zip(parse(_flag(flags, "cnn2_kernel_sizes")), parse(_flag(flags, "cnn2_dilation"))):
        dropped += 2 * dilation * (kernel_size - 1)
    return dropped


class GraphMixedNetLayout(NativeWeights):
    """Any MixedNet flag combination as a conv/BN graph for ``mww_create_convnet`` — the route taken when the
    specialised block kernels do not cover a shape (other filter counts / kernel sizes, ``repeat_in_block`` > 1,
    blocks without a depthwise convolution, ``first_conv_filters`` 0).  Per mixednet.py:307-360:

      first conv  : Conv2D(k1 x 1, stride, valid, no bias) -> ReLU                 -> op(conv, norm none, relu)
      every repeat: MixConv (depthwise + bias, groups fused to one [K_last, C] tap table with structural
                    zero taps, right-aligned like StridedDrop)                      -> op(depthwise, norm bias, linear)
                    Conv2D 1x1 (no bias) -> BatchNormalization -> ReLU              -> op(conv, norm bn, relu)

      residual    : Conv2D 1x1 (no bias) -> BatchNormalization of the block input (mixednet.py:340-345), added to
                    every repeat's BN output before its ReLU after StridedDrop of its leading frames (:354-358)
                                                                                    -> op(conv, norm bn, linear) + ``residual`` links

      heads       : ``spatial_attention`` (SpatialAttention(kernel_size=4), mixednet.py:234-275) and ``pooled`` /
                    ``max_pool`` (global average / max pooling, :372-381) when more than one frame remains -> engine head options
    ``keras_vars`` is ``get_weights()`` order; ``items`` says per op how its native parameter block maps to Keras variables.
    """

    def __init__(self, flags, frames: int):
        topo = MixedNetTopology(flags, frames)
        self.frames = topo.frames
        self.dropout = 0.0
        self.ops: List[dict] = []
        self.op_names: List[str] = []
        self.items: List[dict] = []
        self.keras_vars, self.table = [], []

        cur = -1   # the op whose output the next layer reads

        def op(name, L, kind, norm, act, kernel=1, bn=None, first={}, **last):
            """the op of layer ``L`` on the running tensor with its variables (``bn``: the prefix of its BN's) -> its index"""
            self.ops.append(dict(src=[cur], drop=[0], kernel=kernel, filters=L.cout, **first, norm=norm, act=act, kind=kind,
                                 cin=L.cin, tin=L.tin, tout=L.tout, **last))
            self.op_names.append(name)
            if kind == "depthwise":
                piece = self._mixconv(name[:-len(".dw")], name, L.cin, L.kernel_sizes)
                self.items.append(dict(kind="depthwise", K=piece.K, C=piece.C, groups=piece.groups))
            else:
                shape = (kernel, 1, L.cin, L.cout)
                self.items.append(dict(kind="pw" if bn else "conv", kernel=len(self.keras_vars), shape=shape))
                self._var(name + ".kernel", shape)
                if bn:
                    self._bn(bn, L.cout, name)
            return len(self.ops) - 1

        if topo.conv1:
            if topo.conv1.tout <= 0:
                raise _too_short(frames)
            cur = op("conv1", topo.conv1, "conv", "none", "relu", topo.conv1_kernel, first=dict(stride=topo.stride))
        for bi, (ks, layers) in enumerate(zip(topo.kernels, topo.blocks)):
            _ascending(ks)
            res_op, res_t = None, 0
            for L in layers:
                p = "b%d.r%s" % (bi, L.repeat)
                if L.kind == "res":
                    res_op, res_t = op("b%d.res" % bi, L, "conv", "bn", "linear", bn="b%d.res" % bi), L.tin
                elif L.kind == "mix":
                    if L.tout <= 0:
                        raise _too_short(frames)
                    cur = op(p + ".dw", L, "depthwise", "bias", "linear", max(ks))
                else:
                    cur = op(p + ".pw", L, "conv", "bn", "relu", bn=p, residual=res_op, residual_drop=res_t - L.tin)
        if not self.ops or self.ops[-1]["norm"] != "bn":
            raise NotImplementedError("a MixedNet without any block")
        self.head_attention, self.head_pool, t = topo.head()
        if self.head_attention:
            self._var("attention.kernel", (4, 1, 2, 1))
        self.t_last, self.c_last = t, topo.c_final
        self._var("dense.kernel", (t * topo.c_final, 1))
        self._var("dense.bias", (1,))

    def engine_args(self, max_batch):
        return dict(frames=self.frames, conv_ops=self.ops, dropout=0.0, max_batch=max_batch,
                    head_attention=self.head_attention, head_pool=self.head_pool)

    def summary_lines(self):
        yield "input                                   [B, %d, %d]" % (self.frames, FEATURE_BINS)
        for name, op in zip(self.op_names, self.ops):
            yield "%-12s %-9s %dx1 %s %d->%d, %s, %s   [B, %d, %d]" % (name, op["kind"], op["kernel"], "/%d" % op.get("stride", 1), op["cin"],
                                                                       op["filters"], op["norm"], op["act"], op["tout"], op["filters"])
        head = ("spatial attention(4) + " if self.head_attention else "") + {0: "flatten", 1: "average pool", 2: "max pool"}[self.head_pool]
        yield "%s + dense(1, sigmoid)   [B, 1]" % head
