"""int8 quantization of the streaming MixedNet - the model the reference converts with ``quantize=True``
(microwakeword/utils.py:288-360 ``convert_saved_model_to_tflite``) and evaluates with ``--test_tflite_streaming_quantized``:

  * ``calibrate``   the converter's representative-dataset pass (utils.py:303-325 ``representative_dataset_gen``): one
                    ``get_data("training", 500, ...)`` draw, pixel [0, 0] of the first spectrogram set to 0.0 and [0, 1] to
                    26.0, every spectrogram fed in chunks ``x[i:i+s]`` for ``i in range(0, L - s, s)``.  The calibrator runs
                    one interpreter over all chunks without resetting it, so the pass is one stream-mode run over the
                    concatenated chunks from zero rings; it runs on the float streaming kernel with range recording
                    (``mww_stream_calibrate_host``) and returns every tensor's [min, max].
  * ``quantize``    the int8 parameters from the trained weights and the ranges, per TFLite's int8 quantization spec as the
                    converter applies it to this graph (the contract in INTEGRATION.md): asymmetric per-tensor activations,
                    symmetric per-channel weights, int32 biases, ``QuantizeMultiplier`` requantization, a 256-entry
                    logistic table.  BatchNormalization (eps 1e-3) is folded into the 1x1 weights first.
  * ``QuantizedModel``  those parameters, ``save`` / ``load`` as a data-only ``.npz`` and a readable ``summary``.
  * ``LoopQuantizer``   the int8 model of the CURRENT weights inside the training loop (``quantized: true`` of the
                    ``streaming_validation`` / ``hard_negative_mining`` mappings): a fixed calibration set of windows of
                    resident rows (``calibration_windows``, drawn from generators of its own) calibrated on the device
                    (``mww_stream_calibrate``), then ``quantize_weights`` as above.  The after-training path does not use it.

Nothing here is pinned to TFLite (no TensorFlow on this path); the int8 kernel is pinned to tests/quant_oracle.py.
``plan_ops`` / ``tensor_names`` / ``quantize_weights`` are the one walk over a MixedNet description, residual blocks (kinds
``res`` / ``pw_add``) included: its layer sequence is ``layout.mixednet_layers``, its MixConv fusion ``layout.mixconv_fuse``.
``quantize_mixednet.py`` (residual connections, a pooled head: the normalised description, the refusals, TFLite's int8 Add and
its model class) and ``quantize_graph.py`` (Inception: a graph with concatenations) build on it, on the fixed-point helpers, the
op builders and the ``QuantizedModel`` class below.
"""
from __future__ import annotations

import json
import math
from typing import List, Sequence

import numpy as np

from .layout import FEATURE_BINS, mixconv_fuse, mixednet_layers, split_channels   # noqa: F401 - split_channels: by this name too

BN_EPS = 1e-3
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
CALIBRATION_SAMPLES = 500


# ------------------------------------------------------------------------------------------------ fixed-point helpers

def round_half_away(x):
    """std::round / TfLiteRound: ties away from zero (numpy's round is half-to-even)."""
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def quantize_multiplier(m: float):
    """TFLite ``QuantizeMultiplier``: m = M * 2^(shift - 31) with M in [2^30, 2^31)."""
    m = float(m)
    if m == 0.0:
        return 0, 0
    q, shift = math.frexp(m)
    M = int(round_half_away(q * (1 << 31)))
    if M == (1 << 31):
        M //= 2
        shift += 1
    if shift < -31:
        M = shift = 0
    return M, shift


def srdhm(a: int, b: int) -> int:
    """SaturatingRoundingDoublingHighMul"""
    if a == INT32_MIN and b == INT32_MIN:
        return INT32_MAX
    ab = int(a) * int(b)
    v = ab + ((1 << 30) if ab >= 0 else 1 - (1 << 30))
    return v // (1 << 31) if v >= 0 else -((-v) // (1 << 31))   # C division: truncation


def rdpot(x: int, e: int) -> int:
    """RoundingDivideByPOT"""
    mask = (1 << e) - 1
    r = int(x) & mask
    t = (mask >> 1) + (1 if x < 0 else 0)
    return (int(x) >> e) + (1 if r > t else 0)


def mbqm(x: int, M: int, shift: int) -> int:
    """MultiplyByQuantizedMultiplier (int32 wrap of the left shift)"""
    left, right = max(shift, 0), max(-shift, 0)
    y = (int(x) << left) & 0xFFFFFFFF
    y = y - (1 << 32) if y >= (1 << 31) else y
    return rdpot(srdhm(y, M), right)


def activation_params(rmin: float, rmax: float):
    """Asymmetric int8 parameters of a calibrated range (TFLite GetAsymmetricQuantizationParams / the calibrator's
    nudging): the range widened to hold 0, scale = (rmax - rmin) / 255 in double, the zero point from whichever end has
    the smaller error, rounded half away from zero and clamped.  Returns (float32 scale, int zero point)."""
    rmin, rmax = min(float(rmin), 0.0), max(float(rmax), 0.0)
    if rmin == 0.0 and rmax == 0.0:
        return np.float32(1.0), 0
    scale = (rmax - rmin) / 255.0
    zp_min, zp_max = -128.0 - rmin / scale, 127.0 - rmax / scale
    err_min, err_max = 128.0 + abs(rmin / scale), 127.0 + abs(rmax / scale)
    zp = zp_min if err_min < err_max else zp_max
    zp = -128 if zp < -128 else (127 if zp > 127 else int(round_half_away(zp)))
    return np.float32(scale), int(zp)


def weight_params(w: np.ndarray, axis: int):
    """Symmetric narrow-range per-channel int8 weights along ``axis``: scale_c = max|w_c| / 127 (1 for an all-zero
    channel), q = clamp(round_half_away(w / scale_c), -127, 127).  Returns (int8 q, float32 scales)."""
    w = np.asarray(w, np.float32)
    red = tuple(i for i in range(w.ndim) if i != axis)
    amax = np.abs(w.astype(np.float64)).max(axis=red) if w.size else np.zeros(w.shape[axis])
    scale = np.where(amax > 0, amax / 127.0, 1.0).astype(np.float32)
    shape = [1] * w.ndim
    shape[axis] = -1
    q = np.clip(round_half_away(w.astype(np.float64) / scale.astype(np.float64).reshape(shape)), -127, 127)
    return q.astype(np.int8), scale


def bias_q(b, s_in, s_w):
    """int32 bias: round_half_away(b / (s_in * s_w_c))"""
    v = round_half_away(np.asarray(b, np.float64) / (np.float64(s_in) * np.asarray(s_w, np.float64)))
    return np.clip(v, INT32_MIN, INT32_MAX).astype(np.int64)


def logistic_table(s_in, zp_in) -> np.ndarray:
    """TFLite LUTPopulate for the int8 Logistic (output scale 1/256, zero point -128), in float32, then + 128 (the uint8
    output of inference_output_type=uint8).  Entry v + 128 is the uint8 output of logit q = v."""
    v = np.arange(-128, 128, dtype=np.int32)
    x = np.float32(s_in) * (v - np.int32(zp_in)).astype(np.float32)
    with np.errstate(over="ignore"):
        y = np.float32(1.0) / (np.float32(1.0) + np.exp(-x))
    q = round_half_away(y * np.float32(256.0)).astype(np.int64) - 128   # std::round of the exact y * 256
    return (np.clip(q, -128, 127) + 128).astype(np.uint8)


def fold_bn(kernel, gamma, beta, mean, var):
    """1x1 kernel [Ci, Co] and BN (moving statistics) -> float32 weights and bias, in double as the float stream does"""
    sc = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + BN_EPS)
    w = (np.asarray(kernel, np.float64) * sc[None, :]).astype(np.float32)
    b = (np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * sc).astype(np.float32)
    return w, b


# ---------------------------------------------------------------------------------------------------- the graph

def plan_ops(desc: dict):
    """The plan's layers of a stream description (``layout.mixednet_layers`` behind conv1; ``residual`` defaults to none):
    [(kind, block, repeat, kernel sizes, cin, cout)], kind "res" (a block's residual 1x1, repeat None), "mix" (MixConv, only
    when its largest kernel exceeds 1), "pw" (1x1 + ReLU) or "pw_add" (linear 1x1, then ADD + ReLU)."""
    blocks = [(int(rep), [int(k) for k in ks], int(f)) for rep, ks, f in desc["blocks"]]
    return mixednet_layers(int(desc["conv1_filters"]), blocks, desc.get("residual") or [0] * len(blocks))


def tensor_names(desc: dict) -> List[str]:
    """the calibrated tensors in order: a "res" adds ``block{b}.residual``, a "pw_add" its ADD output behind its 1x1's"""
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


def _r4(n):
    return (n + 3) & ~3


OP_KEYS = ("weights", "weight_scales", "bias", "multiplier", "shift")


def checked_ranges(ranges, n) -> np.ndarray:
    """the calibrated ranges as float64 [n, 2], finite"""
    ranges = np.asarray(ranges, np.float64).reshape(-1, 2)
    if ranges.shape[0] != n:
        raise ValueError("expected %d calibrated ranges, got %d" % (n, ranges.shape[0]))
    if not np.all(np.isfinite(ranges)):
        raise ValueError("a calibrated range is not finite (was the calibration set empty?)")
    return ranges


def activation_table(ranges):
    """``activation_params`` of every range: (float32 scales, int32 zero points)"""
    params = [activation_params(lo, hi) for lo, hi in ranges]
    return np.array([p[0] for p in params], np.float32), np.array([p[1] for p in params], np.int32)


def requant_op(scales, kind, wq, ws, b, t_in, t_out, tensors=None):
    """the dict of one op (``QuantizedModel``): its bias in units of s_in * s_w and, per output channel, the
    ``quantize_multiplier`` of s_in * s_w / s_out in double"""
    s_in, s_out = np.float64(scales[t_in]), np.float64(scales[t_out])
    mult = [quantize_multiplier(s_in * np.float64(sw) / s_out) for sw in ws]
    return dict(kind=kind, weights=wq, weight_scales=ws, bias=bias_q(b, scales[t_in], ws).astype(np.int32),
                multiplier=np.array([m for m, _ in mult], np.int32), shift=np.array([s for _, s in mult], np.int32),
                tensors=tensors or (t_in, t_out))


def fold_mixconv(it, ks, ci):
    """the next MixConv groups of ``it`` (per group kernel [k,1,gc,1] and bias) as one [K, ci] table, taps right-aligned, and
    the bias [ci]"""
    return mixconv_fuse(list(zip(split_channels(ci, len(ks)), ks)), it)


def pointwise_op(scales, it, kind, ci, co, t_in, t_out):
    """the next 1x1 layer of ``it`` (kernel [1,1,ci,co], BN gamma / beta / moving mean / moving variance), BN folded"""
    kern = next(it).reshape(ci, co)
    gamma, beta, mean, var = (next(it).reshape(co) for _ in range(4))
    fw, fb = fold_bn(kern, gamma, beta, mean, var)
    wq, ws = weight_params(fw, 1)
    return requant_op(scales, kind, wq, ws, fb, t_in, t_out)


def dense_op(scales, it, c_last, t_in, t_out, tensors=None, td=None):
    """the Dense of ``it`` (kernel [td * c_last, 1], bias; the last weights) over ``td`` frames (default: what the kernel holds)"""
    dk = next(it).reshape(-1)
    db = next(it).reshape(1)
    if td is not None and dk.size != td * c_last:
        raise ValueError("the dense kernel has %d weights, the description asks for %d" % (dk.size, td * c_last))
    wq, ws = weight_params(dk.reshape(-1, 1), 1)
    return requant_op(scales, "dense", wq.reshape(td or dk.size // c_last, c_last), ws, db, t_in, t_out, tensors)


def _rows_r4(w):
    """int8 rows padded to 32-bit words, flat"""
    n, c = w.shape
    blk = np.zeros((n, _r4(c)), np.int8)
    blk[:, :c] = w
    return blk.reshape(-1)


class QuantizedModel:
    """int8 parameters of a streaming MixedNet.  Per tensor (``names``): ``scales`` float32, ``zero_points`` int32.  Per op
    (conv1, the plan's layers, dense) in ``ops``: dict(kind, weights int8 in the op's natural layout - conv1 [k1*40, C1],
    mix [K, C] (taps right-aligned), pw [Ci, Co], dense [T_f, C] -, weight_scales float32 [cout], bias int32 [cout]
    (without the input zero point), multiplier int32 [cout], shift int32 [cout], tensors (in, out)); ``lut`` uint8 [256].

    Also the base of ``quantize_mixednet.QuantizedMixedNetModel`` (kinds res and pw_add, the latter with ``add`` /
    ``add_tensors``) and ``quantize_graph.QuantizedGraphModel`` (its own ``packed``): a subclass sets ``FAMILY`` (the file's
    ``family`` key; a plain MixedNet file has none) and overrides ``_describe`` / ``_check_family`` / ``_summary_notes``."""

    FAMILY = None
    NAME_WIDTH = 24   # of ``summary``

    def __init__(self, desc, scales, zero_points, ops, lut, ranges=None):
        self.desc, self.names = self._describe(desc)
        self.scales = np.asarray(scales, np.float32)
        self.zero_points = np.asarray(zero_points, np.int32)
        self.ops = ops
        self.lut = np.asarray(lut, np.uint8)
        self.ranges = None if ranges is None else np.asarray(ranges, np.float32)

    @staticmethod
    def _describe(desc):
        """(the description as the model keeps it, the tensor names)"""
        desc = dict(desc)
        return desc, tensor_names(desc)

    # -- the native layout (include/mww.h, mww_stream_set_quantized; residual / pooled: on a stream of mww_stream_create_mixednet_q8)
    def packed(self):
        """(int8 weights, int32 values, input scale, lut) in the layout of mww_stream_set_quantized"""
        wparts, iparts, at = [], [], 0
        for op in self.ops:
            w = op["weights"]
            wsum = w.astype(np.int64).sum(axis=0)
            if op["kind"] == "conv1":
                blk = np.ascontiguousarray(w.T).reshape(-1)                       # [C1][k1*40]
            elif op["kind"] == "mix":
                blk = w.reshape(-1)                                               # [K][C]
            elif op["kind"] in ("pw", "pw_add", "res"):
                blk = _rows_r4(w.T)                                               # [Co][r4(Ci)]
            else:
                blk = _rows_r4(w)                                                 # [T_f or 1][r4(C)]
                wsum = np.array([wsum.sum()], np.int64)
            pad = _r4(at + blk.size) - (at + blk.size)
            wparts += [blk, np.zeros(pad, np.int8)]
            at += blk.size + pad
            folded = self._int32(op["bias"].astype(np.int64) - int(self.zero_points[op["tensors"][0]]) * wsum, op["kind"])
            iparts += [folded, op["multiplier"].astype(np.int64), op["shift"].astype(np.int64)]
            if "add" in op:
                iparts.append(op["add"].astype(np.int64))
        return self._packed(wparts, iparts)

    def _packed(self, wparts, iparts):
        iparts = iparts + [self.zero_points.astype(np.int64)]
        return (np.concatenate(wparts).astype(np.int8), np.concatenate(iparts).astype(np.int32), np.float32(self.scales[0]),
                self.lut)

    @staticmethod
    def _int32(v, what):
        if v.min(initial=0) < INT32_MIN or v.max(initial=0) > INT32_MAX:
            raise OverflowError("folded bias of %s exceeds int32" % what)
        return v

    # -- file
    def save(self, path):
        arrays = {"family": np.array(self.FAMILY)} if self.FAMILY else {}
        arrays.update({"desc": np.array(json.dumps(self.desc)), "names": np.array(self.names), "scales": self.scales,
                       "zero_points": self.zero_points, "lut": self.lut})
        if self.ranges is not None:
            arrays["ranges"] = self.ranges
        for i, op in enumerate(self.ops):
            arrays["op%d/kind" % i] = np.array(op["kind"])
            arrays["op%d/tensors" % i] = np.asarray(op["tensors"], np.int32)
            for k in OP_KEYS:
                arrays["op%d/%s" % (i, k)] = op[k]
            if "add" in op:
                arrays["op%d/add" % i] = op["add"]
                arrays["op%d/add_tensors" % i] = np.asarray(op["add_tensors"], np.int32)
        np.savez(path, **arrays)

    @classmethod
    def _check_family(cls, path, family):
        """raises when the file's ``family`` (None: it has no such key) is not this class's; a plain MixedNet file is not checked"""

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cls._check_family(path, str(z["family"]) if "family" in z.files else None)
            desc = json.loads(str(z["desc"]))
            ops, i = [], 0
            while "op%d/kind" % i in z.files:
                op = {"kind": str(z["op%d/kind" % i]), "tensors": tuple(int(t) for t in z["op%d/tensors" % i])}
                for k in OP_KEYS:
                    op[k] = z["op%d/%s" % (i, k)]
                if "op%d/add" % i in z.files:
                    op["add"] = z["op%d/add" % i]
                    op["add_tensors"] = tuple(int(t) for t in z["op%d/add_tensors" % i])
                ops.append(op)
                i += 1
            return cls(desc, z["scales"], z["zero_points"], ops, z["lut"], z["ranges"] if "ranges" in z.files else None)

    def _summary_notes(self) -> List[str]:
        """lines between the tensors and the output"""
        return []

    def summary(self) -> str:
        name = "%%-%ds" % self.NAME_WIDTH
        lines = [(name + " %14s %11s") % ("tensor", "scale", "zero_point")]
        for n, s, z in zip(self.names, self.scales, self.zero_points):
            lines.append((name + " %14.8g %11d") % (n, float(s), int(z)))
        lines += self._summary_notes()
        lines.append((name + " %14.8g %11d") % ("output (uint8)", 1.0 / 256.0, 0))
        return "\n".join(lines)


def quantize_weights(desc: dict, weights: Sequence[np.ndarray], ranges, model_class=QuantizedModel, dense_frames=None) -> QuantizedModel:
    """The int8 model (a ``model_class``) of a stream description, its Keras-order float weights (``Model.get_weights()``: conv1
    kernel; per block: the residual's 1x1 kernel and BN gamma / beta / moving mean / moving variance when it has one, then per
    repeat each MixConv group's kernel [k,1,gc,1] and bias, the 1x1 kernel and its BN; dense kernel [T_f*C, 1] and bias) and
    the calibrated ranges [n_tensors, 2].  ``dense_frames``: the frames the Dense must cover (default: what its kernel holds)."""
    from .quantize_mixednet import add_params   # (that module imports this one)
    names = tensor_names(desc)
    ranges = checked_ranges(ranges, len(names))
    scales, zps = activation_table(ranges)
    it = iter(np.asarray(a, np.float32) for a in weights)
    k1 = int(desc["conv1_kernel"])
    c1 = int(desc["conv1_filters"])
    wq, ws = weight_params(next(it).reshape(k1 * FEATURE_BINS, c1), 1)            # [k1,1,40,C1]
    ops = [requant_op(scales, "conv1", wq, ws, np.zeros(c1, np.float32), 0, 1)]
    t_in, t, t_res = 1, 2, None   # the tensor the next layer reads, the next tensor, the current block's residual
    for kind, b, r, ks, ci, co in plan_ops(desc):
        if kind == "res":
            ops.append(pointwise_op(scales, it, "res", ci, co, t_in, t))
            t_res = t
            t += 1
            continue
        if kind == "mix":
            fw, fb = fold_mixconv(it, ks, ci)
            wq, ws = weight_params(fw, 1)
            ops.append(requant_op(scales, "mix", wq, ws, fb, t_in, t))
        else:
            ops.append(pointwise_op(scales, it, kind, ci, co, t_in, t))
        if kind == "pw_add":
            ops[-1]["add_tensors"] = (t, t_res, t + 1)
            ops[-1]["add"] = add_params(scales[t], scales[t_res], scales[t + 1], names[t + 1])
            t += 1
        t_in = t
        t += 1
    ops.append(dense_op(scales, it, int(desc["blocks"][-1][2]), t_in, t, td=dense_frames))
    assert t == len(names) - 1
    if next(it, None) is not None:
        raise ValueError("more weights than the stream description holds")
    lut = logistic_table(scales[-1], zps[-1])
    return model_class(desc, scales, zps, ops, lut, ranges.astype(np.float32))


# ---------------------------------------------------------------------------------------- calibration / public API

def calibration_frames(data_processor, config) -> np.ndarray:
    """utils.py:303-325 ``representative_dataset_gen`` as one stream: the concatenated chunks of the 500 drawn
    spectrograms, float32 [n, 40]."""
    x, _, _ = data_processor.get_data("training", CALIBRATION_SAMPLES, features_length=config["spectrogram_length"])
    x[0][0, 0] = 0.0   # guarantee one pixel is the preprocessor min
    x[0][0, 1] = 26.0  # guarantee one pixel is the preprocessor max
    s = int(config["stride"])
    parts = []
    for spectrogram in x:
        n = len(range(0, spectrogram.shape[0] - s, s))
        parts.append(np.asarray(spectrogram[:n * s], np.float32))
    return np.concatenate(parts + [np.zeros((0, FEATURE_BINS), np.float32)], 0)


def refuse_inception(model):
    from .layout import InceptionLayout
    if isinstance(getattr(model, "layout", None), InceptionLayout):
        raise NotImplementedError("this module's int8 evaluation covers MixedNet only (an Inception model is calibrated and quantized by "
                                  "quantize_graph.calibrate / quantize_graph.quantize)")


def _mixednet_only(model):
    from .streaming import mixednet_variant_flags
    refuse_inception(model)
    if mixednet_variant_flags(model.flags):   # before any device work: the float stream of such a model takes no int8 parameters
        raise NotImplementedError("the int8 quantized streaming evaluation does not cover MixedNet with "
                                  + ", ".join(mixednet_variant_flags(model.flags))
                                  + " in this module (quantize_mixednet.calibrate / quantize_mixednet.quantize restate TFLite's int8 "
                                  "ADD and pooling for residual_connection and pooled; int8 MUL is not restated)")


def calibrate(model, data_processor, config) -> np.ndarray:
    """The calibrated [min, max] of every tensor (``tensor_names``) of ``model`` (a trained MixedNet
    ``microwakeword_amd.model.Model``): one stream-mode run of the float streaming kernel from zero rings over
    ``calibration_frames``.  Returns float32 [n_tensors, 2]."""
    from .streaming import StreamingModel
    _mixednet_only(model)
    frames = calibration_frames(data_processor, config)
    sm = StreamingModel(model, int(config["stride"]), "stream")
    return sm.native.calibrate_host(frames)


def quantize(model, ranges) -> QuantizedModel:
    """``quantize_weights`` of a trained MixedNet ``model`` at its own stride."""
    from .layout import _flag
    from .streaming import stream_description
    _mixednet_only(model)
    lay = model.layout
    desc = stream_description(model.flags, lay.t_last, lay.frames, int(_flag(model.flags, "stride")), "stream")
    return quantize_weights(desc, model.get_weights(), ranges)


# ------------------------------------------------------------- the int8 model inside the training loop
# The keys ``streaming_validation`` and ``hard_negative_mining`` share, with their defaults
LOOP_DEFAULTS = dict(quantized=False, calibration_samples=CALIBRATION_SAMPLES, calibration_seed=0)
FORCED_INPUT_RANGE = (0.0, 26.0)   # the two pixels ``calibration_frames`` forces (utils.py:308-309): the preprocessor's min and max


def loop_settings(key, settings):
    """``quantized`` / ``calibration_samples`` / ``calibration_seed`` of a loop option's mapping ``settings``, checked and
    normalised in place; a ``ValueError`` names ``key`` and the bad key.  A mapping that gives none of the three is returned as it
    is - the normalised mapping of a configuration from before these keys stays what it was -, so read them with
    ``settings.get("quantized")``; one that gives any gets the defaults of the others."""
    if not any(k in settings for k in LOOP_DEFAULTS):
        return settings
    for k, default in LOOP_DEFAULTS.items():
        settings.setdefault(k, default)
    q, n, seed = settings["quantized"], settings["calibration_samples"], settings["calibration_seed"]
    integer = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))   # noqa: E731
    bad = [k for k, ok in (("quantized", isinstance(q, (bool, np.bool_))), ("calibration_samples", integer(n) and n >= 1),
                           ("calibration_seed", integer(seed) and 0 <= seed < 2 ** 32)) if not ok]
    if bad:
        raise ValueError("%s: %s out of range (quantized true or false; calibration_samples an integer >= 1; calibration_seed an "
                         "integer in 0 .. 2^32 - 1)" % (key, ", ".join(bad)))
    settings.update(quantized=bool(q), calibration_samples=int(n), calibration_seed=int(seed))
    return settings


def calibration_windows(data_processor, config, samples=CALIBRATION_SAMPLES, seed=0) -> np.ndarray:
    """The calibration set of the loop quantizer as window descriptors of rows that are already resident: the ``windows`` of
    one ``"training"`` draw of ``samples`` spectrograms (``FeatureHandler.draw_seeded_windows``: both MT19937 states built from
    ``seed``, mined providers skipped; no global or private generator moves), each cut to the frames
    ``representative_dataset_gen`` feeds (utils.py:303-325): its first ``n * stride`` rows, ``n = len(range(0, T - stride,
    stride))``.  The cut comes off the end: ``pad_rows`` stays, ``copy_rows`` shrinks.  ``T % stride != 0`` is a ValueError (the
    reference asserts it); an Inception model is fed one frame per step: pass ``dict(config, stride=1)``."""
    T, s = int(config["spectrogram_length"]), int(config["stride"])
    if s < 1 or T % s:
        raise ValueError("spectrogram_length %d is not a multiple of the stride %d" % (T, s))
    if int(samples) < 1:
        raise ValueError("calibration_samples must be >= 1")
    win = data_processor.draw_seeded_windows(int(samples), T, seed)
    keep = len(range(0, T - s, s)) * s
    cut = win["pad_rows"].astype(np.int64) + win["copy_rows"] - keep   # rows off the end (a draw holds T rows per window)
    if np.any(cut < 0):
        raise ValueError("a drawn window holds fewer than %d rows" % keep)
    win["pad_rows"] = np.minimum(win["pad_rows"], keep)
    win["copy_rows"] = keep - win["pad_rows"]
    return win


def window_host_rows(data_processor, windows) -> np.ndarray:
    """``windows`` (descriptors of resident rows) as the float32 [n, 40] frames the device serves, concatenated: zero rows for
    ``pad_rows``, u16 stores scaled by 0.0390625 (``MinedFeatureProvider.host_rows``)."""
    by_id = {int(sid): (p, key) for p in data_processor.feature_providers if getattr(p, "flat", None) for key, sid in p.store_id.items()}
    parts = [np.zeros((0, FEATURE_BINS), np.float32)]
    for w in np.asarray(windows).reshape(-1):
        p, key = by_id[int(w["store"])]
        rows, elem = int(w["copy_rows"]), int(w["src_elem"])
        a = p.flat[key][elem:elem + rows * FEATURE_BINS].reshape(rows, FEATURE_BINS)
        parts.append(np.zeros((int(w["pad_rows"]), FEATURE_BINS), np.float32))
        parts.append(a.astype(np.float32) * np.float32(0.0390625) if key == "u16" else a.astype(np.float32))
    return np.concatenate(parts, 0)


def widen_input_range(ranges) -> np.ndarray:
    """The calibrated ranges with the input tensor's widened to include ``FORCED_INPUT_RANGE``: resident rows cannot carry the two
    pixels ``calibration_frames`` forces, so the loop quantizer states their effect on the range instead."""
    r = np.array(ranges, np.float32).reshape(-1, 2)
    r[0, 0] = min(r[0, 0], np.float32(FORCED_INPUT_RANGE[0]))
    r[0, 1] = max(r[0, 1], np.float32(FORCED_INPUT_RANGE[1]))
    return r


class LoopQuantizer:
    """The int8 model of ``model``'s CURRENT weights at a training step (``at``), for ``streaming_validation`` and
    ``hard_negative_mining`` with ``quantized: true``.  The family module is picked as ``model_train_eval`` picks it
    (``quantize`` for a plain MixedNet, ``quantize_mixednet`` for residual connections / a pooled head, ``quantize_graph`` for
    Inception); its ``NotImplementedError`` for spatial attention and ``first_conv_filters = 0`` is raised here, before any device
    work.  The calibration set (``calibration_windows``) is drawn once, here, from generator states of its own; ``at`` draws
    nothing.  ONE int8-capable stream on the model's context, created at first use, serves every calibration
    (``native.Stream.calibrate``: the ranges are reduced on the device)."""

    def __init__(self, model, data_processor, config, samples=CALIBRATION_SAMPLES, seed=0):
        from . import quantize_graph, quantize_mixednet
        from .layout import InceptionLayout, _flag
        from .streaming import mixednet_variant_flags, stream_description
        self.model = model
        self.samples, self.seed = int(samples), int(seed)
        self.graph = isinstance(getattr(model, "layout", None), InceptionLayout)
        if self.graph:
            self.module, self.int8 = quantize_graph, True
            self.desc = quantize_graph._description(model)
            config = dict(config, stride=1)
        elif mixednet_variant_flags(model.flags):
            self.module, self.int8 = quantize_mixednet, True
            self.desc = quantize_mixednet._description(model, config["stride"])   # refuses attention and first_conv_filters = 0
        else:
            import sys
            self.module, self.int8 = sys.modules[__name__], False
            lay = model.layout
            self.desc = stream_description(model.flags, lay.t_last, lay.frames, int(_flag(model.flags, "stride")), "stream")
        self.stride = int(self.desc["stride"])
        self.windows = calibration_windows(data_processor, config, self.samples, self.seed)
        self.stream = None
        self.calibrations = 0
        self.ranges = None      # of the last calibration, widened
        self._cached = None     # (step, quantized model)

    def close(self):
        if self.stream is not None:
            self.stream.close()
            self.stream = None

    def calibrate(self) -> np.ndarray:
        """the widened ranges of the model's current weights: float rings to zeros, one ``calibrate`` over the windows"""
        from . import native
        if self.stream is None:
            self.stream = (native.GraphStream if self.graph else native.Stream)(self.model.engine, self.desc, int8=self.int8)
        st = self.stream
        st.set_weights(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in self.model.get_weights()]))
        st.reset()
        _, ranges = st.calibrate(self.windows)
        self.calibrations += 1
        self.ranges = widen_input_range(ranges)
        return self.ranges

    def at(self, step):
        """the ``Quantized*Model`` of the current weights, calibrated and quantized once per ``step`` however many ask"""
        if self._cached is None or self._cached[0] != int(step):
            ranges = self.calibrate()
            self._cached = (int(step), self.module.quantize_weights(self.desc, self.model.get_weights(), ranges))
        return self._cached[1]


def check_shared_calibration(*mappings):
    """the loop options' mappings (None: not configured) that say ``quantized`` must name one calibration set: ValueError"""
    sets = {(m["calibration_samples"], m["calibration_seed"]) for m in mappings if m is not None and m.get("quantized")}
    if len(sets) > 1:
        raise ValueError("streaming_validation and hard_negative_mining are both quantized and disagree on calibration_samples / "
                         "calibration_seed (%s): they share one calibration set" % " against ".join("%d / %d" % s for s in sorted(sets)))


def loop_quantizer(owner_key, settings, model, data_processor, config, shared=None):
    """The ``LoopQuantizer`` of a loop option whose mapping says ``quantized`` (None otherwise): ``shared`` - the other option's,
    when it has one - is taken when both name the same calibration set, and a disagreement is a ``ValueError``."""
    if not settings.get("quantized"):
        return None
    if shared is not None:
        if (shared.samples, shared.seed) != (settings["calibration_samples"], settings["calibration_seed"]):
            raise ValueError("%s: calibration_samples / calibration_seed (%d / %d) differ from the other quantized loop option's (%d / %d): "
                             "they share one calibration set" % (owner_key, settings["calibration_samples"], settings["calibration_seed"],
                                                                  shared.samples, shared.seed))
        return shared
    return LoopQuantizer(model, data_processor, config, settings["calibration_samples"], settings["calibration_seed"])
