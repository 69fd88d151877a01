"""int8 quantization of a streaming MixedNet with residual connections or a pooled head - the twin of ``quantize.py`` for
the models ``mww_stream_create_mixednet_q8`` serves (csrc/tu_stream_mixednet_q8.hip), with its fixed-point helpers:

  * ``tensor_names``   the calibrated tensors in order: ``input``, ``conv1``; per block ``block{b}.residual`` (when the block
                       has a residual, in front of its repeats); per repeat ``block{b}.r{r}.mixconv`` (when max(ks) > 1),
                       ``block{b}.r{r}.pointwise`` and, in a residual block, ``block{b}.r{r}.add``; ``dense``.
  * ``calibrate``      ``quantize.calibration_frames`` in one stream-mode pass from zero rings on the float kernel with range
                       recording (a kind-3 layer records the 1x1 output before the add and the ADD output as two tensors).
  * ``quantize``       the int8 parameters (the contract: INTEGRATION.md 6, "residual and pooled MixedNets"; every item our
                       reading, not pinned to TFLite): everything of the plain MixedNet contract, a residual block's 1x1 and its
                       ``r`` linear with their own ranges, TFLite's int8 ``Add`` (left_shift 20) with the ReLU fused, and
                       AVERAGE_POOL_2D / MAX_POOL_2D, which share their input's parameters and add no tensor.
  * ``QuantizedMixedNetModel``  those parameters, ``save`` / ``load`` as a data-only ``.npz`` (``family = "mixednet_variant"``).

Spatial attention and ``first_conv_filters = 0`` are refused before any device work.  The int8 kernel is pinned to
tests/quant_mixednet_oracle.py."""
from __future__ import annotations

import json
from typing import List, Sequence

import numpy as np

from .layout import FEATURE_BINS
from .quantize import (INT32_MAX, INT32_MIN, _r4, activation_params, bias_q, calibration_frames, fold_bn, logistic_table,
                       quantize_multiplier, split_channels, weight_params)

FAMILY = "mixednet_variant"
ADD_LEFT_SHIFT = 20   # TFLite int8 Add


def normalized(desc: dict) -> dict:
    """the description with plain lists and ints (what a JSON round trip gives), residual / attention / pool always present;
    with t_final = 1 the head options do nothing (mixednet.py:362) and are dropped"""
    blocks = [[int(rep), [int(k) for k in ks], int(f)] for rep, ks, f in desc["blocks"]]
    tf = int(desc["t_final"])
    pool = desc.get("pool", 0) or 0
    if pool not in (0, "average", "max"):
        pool = {1: "average", 2: "max"}[int(pool)]
    out = dict(conv1_filters=int(desc["conv1_filters"]), conv1_kernel=int(desc["conv1_kernel"]), stride=int(desc["stride"]),
               blocks=blocks, t_final=tf, frames=int(desc.get("frames", 0)),
               residual=[int(bool(r)) for r in (desc.get("residual") or [0] * len(blocks))],
               attention=int(bool(desc.get("attention", 0))) if tf > 1 else 0, pool=pool if tf > 1 else 0)
    if "mode" in desc:
        out["mode"] = desc["mode"]
    if len(out["residual"]) != len(blocks):
        raise ValueError("residual needs one entry per block")
    return out


def _refuse(desc):
    if int(desc["conv1_filters"]) <= 0:
        raise NotImplementedError("the int8 quantized streaming evaluation does not cover MixedNet with first_conv_filters = 0")
    if desc.get("attention"):
        raise NotImplementedError("the int8 quantized streaming evaluation does not cover MixedNet with spatial_attention (the int8 "
                                  "model is a stream-mode model, stream-mode attention has no pinned reading, and TFLite's int8 MUL / "
                                  "Logistic gate is not restated)")


def plan_ops(desc: dict):
    """The plan's layers: [(kind, block, repeat, kernel sizes, cin, cout)], kind "res" (a block's residual 1x1, repeat None),
    "mix" (MixConv, only when its largest kernel exceeds 1), "pw" (1x1 + ReLU) or "pw_add" (linear 1x1, then ADD + ReLU)."""
    d = normalized(desc)
    ops, c = [], d["conv1_filters"]
    for b, ((rep, ks, f), res) in enumerate(zip(d["blocks"], d["residual"])):
        if res:
            ops.append(("res", b, None, ks, c, f))
        for r in range(rep):
            if max(ks) > 1:
                ops.append(("mix", b, r, ks, c, c))
            ops.append(("pw_add" if res else "pw", b, r, ks, c, f))
            c = f
    return ops


def tensor_names(desc: dict) -> List[str]:
    names = ["input", "conv1"]
    for kind, b, r, _, _, _ in plan_ops(desc):
        if kind == "res":
            names.append("block%d.residual" % b)
        elif kind == "mix":
            names.append("block%d.r%d.mixconv" % (b, r))
        else:
            names.append("block%d.r%d.pointwise" % (b, r))
            if kind == "pw_add":
                names.append("block%d.r%d.add" % (b, r))
    return names + ["dense"]


def add_params(s1, s2, s_out, name="add"):
    """TFLite's int8 Add preparation (left_shift 20) from the float32 scales, in double: int32 [M1, sh1, M2, sh2, Mo, sho].
    All three multipliers are below one (shifts <= 0); an output multiplier >= 1 is where TFLite aborts."""
    s1, s2, s_out = np.float64(np.float32(s1)), np.float64(np.float32(s2)), np.float64(np.float32(s_out))
    twice_max = 2.0 * max(s1, s2)
    m1, m2, mo = s1 / twice_max, s2 / twice_max, twice_max / ((1 << ADD_LEFT_SHIFT) * s_out)
    if not mo < 1.0:
        raise ValueError("tensor %s: the ADD output multiplier %g is not below one (2 max(s1, s2) / (2^20 s_out); TFLite's int8 Add "
                         "aborts there)" % (name, mo))
    out = []
    for m in (m1, m2, mo):
        M, sh = quantize_multiplier(m)
        assert sh <= 0
        out += [M, sh]
    return np.array(out, np.int32)


_OP_KEYS = ("weights", "weight_scales", "bias", "multiplier", "shift")


class QuantizedMixedNetModel:
    """int8 parameters of a streaming MixedNet with residual blocks / a pooled head.  Per tensor (``names``): ``scales``
    float32, ``zero_points`` int32.  Per op (conv1, the plan's layers, dense) in ``ops``: the dict of
    ``quantize.QuantizedModel`` - kind conv1 / res / mix / pw / pw_add / dense; res and pw_add weights [Ci, Co]; a pooled
    dense [1, C] - and, for pw_add, ``add`` int32 [M1, sh1, M2, sh2, Mo, sho] with ``add_tensors`` (1x1 output, r, ADD
    output).  ``lut`` uint8 [256]."""

    def __init__(self, desc, scales, zero_points, ops, lut, ranges=None):
        self.desc = normalized(desc)
        _refuse(self.desc)
        self.names = tensor_names(self.desc)
        self.scales = np.asarray(scales, np.float32)
        self.zero_points = np.asarray(zero_points, np.int32)
        self.ops = ops
        self.lut = np.asarray(lut, np.uint8)
        self.ranges = None if ranges is None else np.asarray(ranges, np.float32)

    # -- the native layout (include/mww.h, mww_stream_set_quantized)
    def packed(self):
        """(int8 weights, int32 values, input scale, lut) in the layout of mww_stream_set_quantized on a stream of
        mww_stream_create_mixednet_q8"""
        wparts, iparts, at = [], [], 0
        for op in self.ops:
            w = op["weights"]
            if op["kind"] == "conv1":
                blk = np.ascontiguousarray(w.T).reshape(-1)                       # [C1][k1*40]
                wsum = w.astype(np.int64).sum(axis=0)
            elif op["kind"] == "mix":
                blk = w.reshape(-1)                                               # [K][C]
                wsum = w.astype(np.int64).sum(axis=0)
            elif op["kind"] in ("pw", "pw_add", "res"):
                ci, co = w.shape
                blk = np.zeros((co, _r4(ci)), np.int8)
                blk[:, :ci] = w.T
                blk = blk.reshape(-1)                                             # [Co][r4(Ci)]
                wsum = w.astype(np.int64).sum(axis=0)
            else:
                tf, c = w.shape
                blk = np.zeros((tf, _r4(c)), np.int8)
                blk[:, :c] = w
                blk = blk.reshape(-1)                                             # [T_f or 1][r4(C)]
                wsum = np.array([w.astype(np.int64).sum()], np.int64)
            pad = _r4(at + blk.size) - (at + blk.size)
            wparts += [blk, np.zeros(pad, np.int8)]
            at += blk.size + pad
            folded = op["bias"].astype(np.int64) - int(self.zero_points[op["tensors"][0]]) * wsum
            if folded.min(initial=0) < INT32_MIN or folded.max(initial=0) > INT32_MAX:
                raise OverflowError("folded bias of %s exceeds int32" % op["kind"])
            iparts += [folded, op["multiplier"].astype(np.int64), op["shift"].astype(np.int64)]
            if op["kind"] == "pw_add":
                iparts.append(op["add"].astype(np.int64))
        iparts.append(self.zero_points.astype(np.int64))
        return (np.concatenate(wparts).astype(np.int8), np.concatenate(iparts).astype(np.int32), np.float32(self.scales[0]),
                self.lut)

    # -- file
    def save(self, path):
        arrays = {"family": np.array(FAMILY), "desc": np.array(json.dumps(self.desc)), "names": np.array(self.names),
                  "scales": self.scales, "zero_points": self.zero_points, "lut": self.lut}
        if self.ranges is not None:
            arrays["ranges"] = self.ranges
        for i, op in enumerate(self.ops):
            arrays["op%d/kind" % i] = np.array(op["kind"])
            arrays["op%d/tensors" % i] = np.asarray(op["tensors"], np.int32)
            for k in _OP_KEYS:
                arrays["op%d/%s" % (i, k)] = op[k]
            if op["kind"] == "pw_add":
                arrays["op%d/add" % i] = op["add"]
                arrays["op%d/add_tensors" % i] = np.asarray(op["add_tensors"], np.int32)
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "family" not in z.files or str(z["family"]) != FAMILY:
                raise ValueError("%s is not a residual / pooled MixedNet file (family %r)" % (
                    path, str(z["family"]) if "family" in z.files else "mixednet"))
            desc = json.loads(str(z["desc"]))
            ops, i = [], 0
            while "op%d/kind" % i in z.files:
                op = {"kind": str(z["op%d/kind" % i]), "tensors": tuple(int(t) for t in z["op%d/tensors" % i])}
                for k in _OP_KEYS:
                    op[k] = z["op%d/%s" % (i, k)]
                if op["kind"] == "pw_add":
                    op["add"] = z["op%d/add" % i]
                    op["add_tensors"] = tuple(int(t) for t in z["op%d/add_tensors" % i])
                ops.append(op)
                i += 1
            return cls(desc, z["scales"], z["zero_points"], ops, z["lut"], z["ranges"] if "ranges" in z.files else None)

    def summary(self) -> str:
        lines = ["%-24s %14s %11s" % ("tensor", "scale", "zero_point")]
        for n, s, z in zip(self.names, self.scales, self.zero_points):
            lines.append("%-24s %14.8g %11d" % (n, float(s), int(z)))
        if self.desc["pool"]:
            lines.append("%-24s %14s" % ("%s pool over %d" % (self.desc["pool"], self.desc["t_final"]), "(shares its input's)"))
        lines.append("output (uint8)           %14.8g %11d" % (1.0 / 256.0, 0))
        return "\n".join(lines)


def quantize_weights(desc: dict, weights: Sequence[np.ndarray], ranges) -> QuantizedMixedNetModel:
    """The int8 model of an extended stream description (``streaming.mixednet_stream_description``), its Keras-order float
    weights (``Model.get_weights()``: conv1 kernel; per block: the residual's 1x1 kernel and BN gamma / beta / moving mean /
    moving variance when it has one, then per repeat each MixConv group's kernel [k,1,gc,1] and bias, the 1x1 kernel and its
    BN; dense kernel [T_f*C, 1] - pooled: [C, 1] - and bias) and the calibrated ranges [n_tensors, 2]."""
    desc = normalized(desc)
    _refuse(desc)
    w = [np.asarray(a, np.float32) for a in weights]
    ranges = np.asarray(ranges, np.float64).reshape(-1, 2)
    names = tensor_names(desc)
    if ranges.shape[0] != len(names):
        raise ValueError("expected %d calibrated ranges, got %d" % (len(names), ranges.shape[0]))
    if not np.all(np.isfinite(ranges)):
        raise ValueError("a calibrated range is not finite (was the calibration set empty?)")
    params = [activation_params(lo, hi) for lo, hi in ranges]
    scales = np.array([p[0] for p in params], np.float32)
    zps = np.array([p[1] for p in params], np.int32)
    ops = []

    def op(kind, wq, ws, b, t_in, t_out):
        s_in, s_out = np.float64(scales[t_in]), np.float64(scales[t_out])
        mult = [quantize_multiplier(s_in * np.float64(sw) / s_out) for sw in ws]
        ops.append(dict(kind=kind, weights=wq, weight_scales=ws, bias=bias_q(b, scales[t_in], ws).astype(np.int32),
                        multiplier=np.array([m for m, _ in mult], np.int32), shift=np.array([s for _, s in mult], np.int32),
                        tensors=(t_in, t_out)))
        return ops[-1]

    it = iter(w)
    k1, c1 = desc["conv1_kernel"], desc["conv1_filters"]
    wq, ws = weight_params(next(it).reshape(k1 * FEATURE_BINS, c1), 1)                # [k1,1,40,C1]
    op("conv1", wq, ws, np.zeros(c1, np.float32), 0, 1)

    def pointwise(kind, ci, co, t_in, t_out):
        kern = next(it).reshape(ci, co)
        gamma, beta, mean, var = (next(it).reshape(co) for _ in range(4))
        fw, fb = fold_bn(kern, gamma, beta, mean, var)
        wq, ws = weight_params(fw, 1)
        return op(kind, wq, ws, fb, t_in, t_out)

    t_in, t, t_res = 1, 2, None   # the tensor the next layer reads, the next tensor, the current block's residual
    for kind, b, r, ks, ci, co in plan_ops(desc):
        if kind == "res":
            pointwise("res", ci, co, t_in, t)
            t_res = t
            t += 1
        elif kind == "mix":
            K = max(ks)
            fw = np.zeros((K, ci), np.float32)
            fb = np.zeros(ci, np.float32)
            c0 = 0
            for gc, kk in zip(split_channels(ci, len(ks)), ks):
                fw[K - kk:, c0:c0 + gc] = next(it).reshape(kk, gc)
                fb[c0:c0 + gc] = next(it).reshape(gc)
                c0 += gc
            wq, ws = weight_params(fw, 1)
            op("mix", wq, ws, fb, t_in, t)
            t_in = t
            t += 1
        elif kind == "pw":
            pointwise("pw", ci, co, t_in, t)
            t_in = t
            t += 1
        else:
            o = pointwise("pw_add", ci, co, t_in, t)
            o["add_tensors"] = (t, t_res, t + 1)
            o["add"] = add_params(scales[t], scales[t_res], scales[t + 1], names[t + 1])
            t_in = t + 1
            t += 2
    dk = next(it).reshape(-1)
    db = next(it).reshape(1)
    c_last = desc["blocks"][-1][2]
    td = 1 if desc["pool"] else desc["t_final"]
    if dk.size != td * c_last:
        raise ValueError("the dense kernel has %d weights, the description asks for %d" % (dk.size, td * c_last))
    wq, ws = weight_params(dk.reshape(-1, 1), 1)
    op("dense", wq.reshape(td, c_last), ws, db, t_in, t)
    assert t == len(names) - 1
    if next(it, None) is not None:
        raise ValueError("more weights than the stream description holds")
    lut = logistic_table(scales[-1], zps[-1])
    return QuantizedMixedNetModel(desc, scales, zps, ops, lut, ranges.astype(np.float32))


# ---------------------------------------------------------------------------------------- calibration / public API

def _description(model, stride=None):
    """the stream-mode description of a trained MixedNet ``model``; refuses attention and first_conv_filters = 0"""
    from .layout import InceptionLayout, _flag
    from .streaming import mixednet_stream_description
    if isinstance(getattr(model, "layout", None), InceptionLayout):
        raise NotImplementedError("this module's int8 evaluation covers MixedNet only (an Inception model is calibrated and quantized by "
                                  "quantize_graph.calibrate / quantize_graph.quantize)")
    stride = int(_flag(model.flags, "stride")) if stride is None else int(stride)
    return mixednet_stream_description(model.flags, model.layout.frames, stride, "stream")   # raises for both refusals


def calibrate(model, data_processor, config) -> np.ndarray:
    """The calibrated [min, max] of every tensor (``tensor_names``) of ``model`` (a trained MixedNet
    ``microwakeword_amd.model.Model``, residual connections and a pooled head included): one stream-mode run of the float
    streaming kernel from zero rings over ``quantize.calibration_frames`` on a stream of ``mww_stream_create_mixednet_q8``.
    Returns float32 [n_tensors, 2]."""
    from . import native
    desc = _description(model, config["stride"])   # before any device work
    frames = calibration_frames(data_processor, config)
    st = native.Stream(model.engine, desc, int8=True)
    try:
        st.set_weights(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()]))
        return st.calibrate_host(frames)
    finally:
        st.close()


def quantize(model, ranges) -> QuantizedMixedNetModel:
    """``quantize_weights`` of a trained MixedNet ``model`` at its own stride."""
    return quantize_weights(_description(model), model.get_weights(), ranges)
