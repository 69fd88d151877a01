"""int8 quantization of the streaming Inception model - any conv -> BN/SSN -> ReLU graph of ``native.GraphStream`` - the
model the reference converts with ``quantize=True`` (microwakeword/utils.py:288-360; the conversion does not depend on the
model family) and evaluates with ``--test_tflite_streaming_quantized``.  The MixedNet form is ``quantize.py``; the
fixed-point helpers, the op builders and the model class it extends are imported from it.

  * ``calibrate``   the representative-dataset pass as one stream-mode run from zero rings over
                    ``quantize.calibration_frames`` at stride 1 (an Inception model has no ``--stride``), on the float graph
                    kernel with range recording; returns the [min, max] of the ``n_ops + 2`` tensors: the input, every op's
                    output (after folded BN/SSN + ReLU), the Dense logit.
  * ``quantize_weights``  the int8 parameters of a graph description (the contract in INTEGRATION.md):
        folding        BN/SSN (moving statistics, eps 1e-3, channel c -> slot c mod g) folded into each convolution in double
                       and rounded to float32 - the same fold as the float stream's ``set_weights``;
        weights        per output filter, symmetric narrow-range, over [k, Cin]; int32 bias from the folded shift;
        multiplier     s_in * s_w / s_out in double, ``QuantizeMultiplier``;
        concatenation  all sources of an op with more than one source share one (scale, zero point), derived from the union
                       of their calibrated ranges - TFLite's same-scale constraint on CONCATENATION.  The classes are built
                       with a union-find over all multi-source ops, so a tensor that feeds two concatenations merges them;
                       the spectrogram joins a class like any tensor.  Every op then has one s_in / zp_in;
        slices         a channel slice has no parameters of its own: a tensor has one set;
        Dense, table   as the MixedNet path.
  * ``QuantizedGraphModel``  those parameters, ``packed`` (the layout of mww_stream_set_quantized for a graph stream),
                    ``save`` / ``load`` as a data-only ``.npz`` carrying ``family = "graph"``, and a readable ``summary``.

Nothing here is pinned to TFLite; the int8 graph kernel is pinned to tests/quant_graph_oracle.py.
"""
from __future__ import annotations

import json
from typing import List, Sequence

import numpy as np

from .layout import FEATURE_BINS
from .quantize import (BN_EPS, QuantizedModel, _r4, _rows_r4, activation_table, checked_ranges, dense_op, logistic_table,
                       requant_op, round_half_away, weight_params)
from . import quantize as _mixednet

FAMILY = "graph"
__all__ = ["FAMILY", "QuantizedGraphModel", "calibrate", "calibration_frames", "concat_classes", "fold_op", "op_sources",
           "quantize", "quantize_weights", "round_half_away", "tensor_names"]


def op_sources(desc: dict):
    """per op: [(source tensor, first channel, channels)] - tensor 0 is the input, 1 + i the output of op i"""
    ops = desc["conv_ops"]
    ch = [FEATURE_BINS] + [int(o["filters"]) for o in ops]
    out = []
    for op in ops:
        src = list(op["src"])
        sl = list(op.get("slice", [(0, 0)] * len(src)))
        out.append([(int(s) + 1, int(c0), int(cn) if int(cn) else ch[int(s) + 1] - int(c0)) for s, (c0, cn) in zip(src, sl)])
    return out


def tensor_names(desc: dict) -> List[str]:
    names = list(desc.get("op_names") or ["op%d" % i for i in range(len(desc["conv_ops"]))])
    return ["input"] + names + ["dense"]


def concat_classes(desc: dict) -> List[int]:
    """class representative (smallest member) of each of the n_ops + 1 activation tensors: the sources of every op with more
    than one source are merged (union-find)"""
    n = len(desc["conv_ops"]) + 1
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for srcs in op_sources(desc):
        if len(srcs) > 1:
            for t, _, _ in srcs[1:]:
                a, b = find(srcs[0][0]), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return [find(t) for t in range(n)]


def fold_op(op: dict, cin: int, kernel, gamma, beta, mean, var):
    """Keras kernel [k,1,Cin,F] and BN / SSN moving statistics [slots] -> float32 folded weights [k, Cin, F] and bias [F]"""
    k, co, g = int(op["kernel"]), int(op["filters"]), int(op.get("bn_groups", 1))
    slot = np.arange(co) % g if g > 1 else np.arange(co)
    sc = np.asarray(gamma, np.float64)[slot] / np.sqrt(np.asarray(var, np.float64)[slot] + BN_EPS)
    w = (np.asarray(kernel, np.float64).reshape(k, cin, co) * sc[None, None, :]).astype(np.float32)
    b = (np.asarray(beta, np.float64)[slot] - np.asarray(mean, np.float64)[slot] * sc).astype(np.float32)
    return w, b


class QuantizedGraphModel(QuantizedModel):
    """int8 parameters of a streaming conv/BN graph.  Per tensor (``names``: input, every op's output, dense): ``scales``
    float32, ``zero_points`` int32, ``classes`` (the concatenation class of each activation tensor).  Per op in ``ops``:
    dict(kind "conv" / "dense", weights int8 - conv [k, Cin, Co] (sources concatenated along Cin), dense [T_f, C] -,
    weight_scales float32 [cout], bias int32 [cout] (without the input zero point), multiplier, shift int32 [cout],
    tensors = the source tensors then the output tensor); ``lut`` uint8 [256].  ``save`` / ``load`` are the base class's."""

    FAMILY = FAMILY
    NAME_WIDTH = 28

    def __init__(self, desc, scales, zero_points, ops, lut, ranges=None):
        super().__init__(desc, scales, zero_points, ops, lut, ranges)
        self.classes = concat_classes(self.desc)
        self.sources = op_sources(self.desc)

    @staticmethod
    def _describe(desc):
        desc = json.loads(json.dumps(desc))   # a plain copy: tuples become lists, as a loaded file has them
        return desc, tensor_names(desc)

    # -- the native layout (include/mww.h, mww_stream_set_quantized on a stream of mww_stream_create_convnet_q8)
    def packed(self):
        """(int8 weights, int32 values, input scale, lut)"""
        wparts, iparts = [], []
        for op, srcs in zip(self.ops[:-1], self.sources):
            w = op["weights"]                                          # [k, Cin, Co]
            k, _, co = w.shape
            cols, at = [], 0
            folded = op["bias"].astype(np.int64)
            for t, _, cn in srcs:                                     # every source's slice padded to a 4-byte word
                part = np.zeros((k, _r4(cn), co), np.int8)
                part[:, :cn] = w[:, at:at + cn]
                cols.append(part)
                folded = folded - int(self.zero_points[t]) * w[:, at:at + cn].astype(np.int64).sum(axis=(0, 1))
                at += cn
            wparts.append(np.ascontiguousarray(np.concatenate(cols, 1).transpose(2, 0, 1)).reshape(-1))   # [Co][k][kp]
            iparts += [self._int32(folded, "op"), op["multiplier"].astype(np.int64), op["shift"].astype(np.int64)]
        d = self.ops[-1]
        wparts.append(_rows_r4(d["weights"]))
        folded = d["bias"].astype(np.int64) - int(self.zero_points[d["tensors"][0]]) * d["weights"].astype(np.int64).sum()
        iparts += [self._int32(folded, "dense"), d["multiplier"].astype(np.int64), d["shift"].astype(np.int64)]
        return self._packed(wparts, iparts)

    @classmethod
    def _check_family(cls, path, family):
        if family != FAMILY:
            raise ValueError("%s does not hold a quantized graph model (quantize.QuantizedModel.load reads a MixedNet file)" % path)

    def summary(self) -> str:
        lines = super().summary().split("\n")   # + the class column on the header and on every tensor's line
        col = ["class"] + [self.classes[t] if t < len(self.classes) else "-" for t in range(len(self.names))]
        return "\n".join(["%s %6s" % lc for lc in zip(lines, col)] + lines[-1:])


def quantize_weights(desc: dict, weights: Sequence[np.ndarray], ranges) -> QuantizedGraphModel:
    """The int8 model of a graph stream description (``streaming.graph_stream_description``), its Keras-order float weights
    (per op kernel [k,1,Cin,F], gamma, beta, moving mean, moving variance [slots]; dense kernel [T_f*C, 1] and bias) and the
    calibrated ranges [n_ops + 2, 2]."""
    ops_d = desc["conv_ops"]
    n = len(ops_d)
    ranges = checked_ranges(ranges, n + 2)
    # one (scale, zero point) per concatenation class, from the union of its members' ranges
    cls = concat_classes(desc)
    union = ranges.copy()
    for t in range(n + 1):
        members = [m for m in range(n + 1) if cls[m] == cls[t]]
        union[t] = ranges[members, 0].min(), ranges[members, 1].max()
    scales, zps = activation_table(union)
    ops = []
    it = iter(np.asarray(a, np.float32) for a in weights)
    for i, (o, srcs) in enumerate(zip(ops_d, op_sources(desc))):
        cin = sum(cn for _, _, cn in srcs)
        kern, gamma, beta, mean, var = (next(it) for _ in range(5))
        fw, fb = fold_op(o, cin, kern, gamma, beta, mean, var)
        wq, ws = weight_params(fw, 2)
        ops.append(requant_op(scales, "conv", wq, ws, fb, srcs[0][0], 1 + i, tuple(t for t, _, _ in srcs) + (1 + i,)))
    ops.append(dense_op(scales, it, int(ops_d[-1]["filters"]), n, n + 1, (n, n + 1)))
    if next(it, None) is not None:
        raise ValueError("more weights than the graph description holds")
    lut = logistic_table(scales[-1], zps[-1])
    return QuantizedGraphModel(desc, scales, zps, ops, lut, ranges.astype(np.float32))


# ---------------------------------------------------------------------------------------- calibration / public API

def calibration_frames(data_processor, config) -> np.ndarray:
    """``quantize.calibration_frames`` at stride 1: an Inception model is fed one frame per step"""
    return _mixednet.calibration_frames(data_processor, dict(config, stride=1))


def _description(model, mode="stream"):
    from .layout import InceptionLayout
    from .streaming import graph_stream_description
    if not isinstance(getattr(model, "layout", None), InceptionLayout):
        raise NotImplementedError("quantize_graph covers Inception models (quantize.py covers MixedNet)")
    return graph_stream_description(model.flags, model.layout.frames, 1, mode)


def calibrate(model, data_processor, config) -> np.ndarray:
    """The calibrated [min, max] of every tensor (``tensor_names``) of a trained Inception ``model``: one stream-mode pass
    of the float graph kernel from zero rings over ``calibration_frames``.  Returns float32 [n_ops + 2, 2]."""
    from . import native
    frames = calibration_frames(data_processor, config)
    st = native.GraphStream(model.engine, _description(model), int8=True)
    try:
        st.set_weights(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in model.get_weights()]))
        return st.calibrate_host(frames)
    finally:
        st.close()


def quantize(model, ranges) -> QuantizedGraphModel:
    """``quantize_weights`` of a trained Inception ``model``"""
    return quantize_weights(_description(model), model.get_weights(), ranges)
