"""int8 quantization of the streaming Inception model - any conv -> BN/SSN -> ReLU graph of ``native.GraphStream`` - the
model the reference converts with ``quantize=True`` (microwakeword/utils.py:288-360; the conversion does not depend on the
model family) and evaluates with ``--test_tflite_streaming_quantized``.  The MixedNet twin is ``quantize.py``; the
fixed-point helpers are imported from it.

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
from .quantize import (BN_EPS, INT32_MAX, INT32_MIN, activation_params, bias_q, logistic_table, quantize_multiplier,
                       round_half_away, weight_params)
from . import quantize as _mixednet

FAMILY = "graph"
__all__ = ["FAMILY", "QuantizedGraphModel", "calibrate", "calibration_frames", "concat_classes", "fold_op", "op_sources",
           "quantize", "quantize_weights", "round_half_away", "tensor_names"]


def _r4(n):
    return (int(n) + 3) & ~3


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


class QuantizedGraphModel:
    """int8 parameters of a streaming conv/BN graph.  Per tensor (``names``: input, every op's output, dense): ``scales``
    float32, ``zero_points`` int32, ``classes`` (the concatenation class of each activation tensor).  Per op in ``ops``:
    dict(kind "conv" / "dense", weights int8 - conv [k, Cin, Co] (sources concatenated along Cin), dense [T_f, C] -,
    weight_scales float32 [cout], bias int32 [cout] (without the input zero point), multiplier, shift int32 [cout],
    tensors = the source tensors then the output tensor); ``lut`` uint8 [256]."""

    family = FAMILY

    def __init__(self, desc, scales, zero_points, ops, lut, ranges=None):
        self.desc = json.loads(json.dumps(desc))   # a plain copy: tuples become lists, as a loaded file has them
        self.names = tensor_names(self.desc)
        self.scales = np.asarray(scales, np.float32)
        self.zero_points = np.asarray(zero_points, np.int32)
        self.ops = ops
        self.lut = np.asarray(lut, np.uint8)
        self.ranges = None if ranges is None else np.asarray(ranges, np.float32)
        self.classes = concat_classes(self.desc)
        self.sources = op_sources(self.desc)

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
        tf, c = d["weights"].shape
        blk = np.zeros((tf, _r4(c)), np.int8)
        blk[:, :c] = d["weights"]
        wparts.append(blk.reshape(-1))
        zp_in = int(self.zero_points[d["tensors"][0]])
        folded = d["bias"].astype(np.int64) - zp_in * d["weights"].astype(np.int64).sum()
        iparts += [self._int32(folded, "dense"), d["multiplier"].astype(np.int64), d["shift"].astype(np.int64)]
        iparts.append(self.zero_points.astype(np.int64))
        return (np.concatenate(wparts).astype(np.int8), np.concatenate(iparts).astype(np.int32), np.float32(self.scales[0]),
                self.lut)

    @staticmethod
    def _int32(v, what):
        if v.min(initial=0) < INT32_MIN or v.max(initial=0) > INT32_MAX:
            raise OverflowError("folded bias of %s exceeds int32" % what)
        return v

    # -- file
    def save(self, path):
        arrays = {"family": np.array(FAMILY), "desc": np.array(json.dumps(self.desc)), "names": np.array(self.names),
                  "scales": self.scales, "zero_points": self.zero_points, "lut": self.lut}
        if self.ranges is not None:
            arrays["ranges"] = self.ranges
        for i, op in enumerate(self.ops):
            arrays["op%d/kind" % i] = np.array(op["kind"])
            arrays["op%d/tensors" % i] = np.asarray(op["tensors"], np.int32)
            for k in ("weights", "weight_scales", "bias", "multiplier", "shift"):
                arrays["op%d/%s" % (i, k)] = op[k]
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "family" not in z.files or str(z["family"]) != FAMILY:
                raise ValueError("%s does not hold a quantized graph model (quantize.QuantizedModel.load reads a MixedNet file)" % path)
            desc = json.loads(str(z["desc"]))
            ops, i = [], 0
            while "op%d/kind" % i in z.files:
                op = {"kind": str(z["op%d/kind" % i]), "tensors": tuple(int(t) for t in z["op%d/tensors" % i])}
                for k in ("weights", "weight_scales", "bias", "multiplier", "shift"):
                    op[k] = z["op%d/%s" % (i, k)]
                ops.append(op)
                i += 1
            return cls(desc, z["scales"], z["zero_points"], ops, z["lut"], z["ranges"] if "ranges" in z.files else None)

    def summary(self) -> str:
        lines = ["%-28s %14s %11s %6s" % ("tensor", "scale", "zero_point", "class")]
        for t, (n, s, z) in enumerate(zip(self.names, self.scales, self.zero_points)):
            lines.append("%-28s %14.8g %11d %6s" % (n, float(s), int(z), self.classes[t] if t < len(self.classes) else "-"))
        lines.append("%-28s %14.8g %11d" % ("output (uint8)", 1.0 / 256.0, 0))
        return "\n".join(lines)


def quantize_weights(desc: dict, weights: Sequence[np.ndarray], ranges) -> QuantizedGraphModel:
    """The int8 model of a graph stream description (``streaming.graph_stream_description``), its Keras-order float weights
    (per op kernel [k,1,Cin,F], gamma, beta, moving mean, moving variance [slots]; dense kernel [T_f*C, 1] and bias) and the
    calibrated ranges [n_ops + 2, 2]."""
    w = [np.asarray(a, np.float32) for a in weights]
    ops_d = desc["conv_ops"]
    n = len(ops_d)
    ranges = np.asarray(ranges, np.float64).reshape(-1, 2)
    if ranges.shape[0] != n + 2:
        raise ValueError("expected %d calibrated ranges, got %d" % (n + 2, ranges.shape[0]))
    if not np.all(np.isfinite(ranges)):
        raise ValueError("a calibrated range is not finite (was the calibration set empty?)")
    # one (scale, zero point) per concatenation class, from the union of its members' ranges
    cls = concat_classes(desc)
    params = []
    for t in range(n + 1):
        members = [m for m in range(n + 1) if cls[m] == cls[t]]
        params.append(activation_params(ranges[members, 0].min(), ranges[members, 1].max()))
    params.append(activation_params(*ranges[n + 1]))
    scales = np.array([p[0] for p in params], np.float32)
    zps = np.array([p[1] for p in params], np.int32)
    sources = op_sources(desc)
    ops = []

    def op(kind, wq, ws, b, t_in, t_out):
        s_in, s_out = np.float64(scales[t_in[0]]), np.float64(scales[t_out])
        mult = [quantize_multiplier(s_in * np.float64(sw) / s_out) for sw in ws]
        ops.append(dict(kind=kind, weights=wq, weight_scales=ws, bias=bias_q(b, scales[t_in[0]], ws).astype(np.int32),
                        multiplier=np.array([m for m, _ in mult], np.int32), shift=np.array([s for _, s in mult], np.int32),
                        tensors=tuple(t_in) + (t_out,)))

    it = iter(w)
    for i, (o, srcs) in enumerate(zip(ops_d, sources)):
        cin = sum(cn for _, _, cn in srcs)
        kern, gamma, beta, mean, var = (next(it) for _ in range(5))
        fw, fb = fold_op(o, cin, kern, gamma, beta, mean, var)
        wq, ws = weight_params(fw, 2)
        op("conv", wq, ws, fb, [t for t, _, _ in srcs], 1 + i)
    dk = next(it).reshape(-1)
    db = next(it).reshape(1)
    c_last = int(ops_d[-1]["filters"])
    tf = dk.size // c_last
    wq, ws = weight_params(dk.reshape(-1, 1), 1)
    op("dense", wq.reshape(tf, c_last), ws, db, [n], n + 1)
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
