"""int8 quantization of a streaming MixedNet with residual connections or a pooled head - ``quantize.py`` extended to the
models ``mww_stream_create_mixednet_q8`` serves (the <VAR> kernel of csrc/tu_stream_q8.hip), on its helpers and its model class:

  * ``tensor_names``   (``quantize.tensor_names``; like ``plan_ops`` the one definition) the calibrated tensors in order:
                       ``input``, ``conv1``; per block ``block{b}.residual`` (when the block has a residual, in front of its repeats); per repeat ``block{b}.r{r}.mixconv`` (when max(ks) > 1),
                       ``block{b}.r{r}.pointwise`` and, in a residual block, ``block{b}.r{r}.add``; ``dense``.
  * ``calibrate``      ``quantize.calibration_frames`` in one stream-mode pass from zero rings on the float kernel with range
                       recording (a kind-3 layer records the 1x1 output before the add and the ADD output as two tensors).
  * ``quantize``       (``quantize.quantize_weights`` on the normalised description) the int8 parameters (the contract:
                       INTEGRATION.md 6, "residual and pooled MixedNets"; every item our reading, not pinned to TFLite): everything of the plain MixedNet contract, a residual block's 1x1 and its
                       ``r`` linear with their own ranges, TFLite's int8 ``Add`` (left_shift 20) with the ReLU fused, and
                       AVERAGE_POOL_2D / MAX_POOL_2D, which share their input's parameters and add no tensor.
  * ``QuantizedMixedNetModel``  those parameters, ``save`` / ``load`` as a data-only ``.npz`` (``family = "mixednet_variant"``).

Spatial attention and ``first_conv_filters = 0`` are refused before any device work.  The int8 kernel is pinned to
tests/quant_mixednet_oracle.py."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import quantize as _plain
from .quantize import QuantizedModel, calibration_frames, plan_ops, quantize_multiplier, refuse_inception, tensor_names   # noqa: F401

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


class QuantizedMixedNetModel(QuantizedModel):
    """int8 parameters of a streaming MixedNet with residual blocks / a pooled head.  Per tensor (``names``): ``scales``
    float32, ``zero_points`` int32.  Per op (conv1, the plan's layers, dense) in ``ops``: the dict of
    ``quantize.QuantizedModel`` - kind conv1 / res / mix / pw / pw_add / dense; res and pw_add weights [Ci, Co]; a pooled
    dense [1, C] - and, for pw_add, ``add`` int32 [M1, sh1, M2, sh2, Mo, sho] with ``add_tensors`` (1x1 output, r, ADD
    output).  ``lut`` uint8 [256].  ``packed`` / ``save`` / ``load`` are the base class's (the file carries ``family``)."""

    FAMILY = FAMILY

    @staticmethod
    def _describe(desc):
        desc = normalized(desc)
        _refuse(desc)
        return desc, tensor_names(desc)

    @classmethod
    def _check_family(cls, path, family):
        if family != FAMILY:
            raise ValueError("%s is not a residual / pooled MixedNet file (family %r)" % (path, family or "mixednet"))

    def _summary_notes(self):
        if not self.desc["pool"]:
            return []
        return ["%-24s %14s" % ("%s pool over %d" % (self.desc["pool"], self.desc["t_final"]), "(shares its input's)")]


def quantize_weights(desc: dict, weights: Sequence[np.ndarray], ranges) -> QuantizedMixedNetModel:
    """The int8 model of an extended stream description (``streaming.mixednet_stream_description``), its Keras-order float
    weights (``Model.get_weights()``: conv1 kernel; per block: the residual's 1x1 kernel and BN gamma / beta / moving mean /
    moving variance when it has one, then per repeat each MixConv group's kernel [k,1,gc,1] and bias, the 1x1 kernel and its
    BN; dense kernel [T_f*C, 1] - pooled: [C, 1] - and bias) and the calibrated ranges [n_tensors, 2]."""
    desc = normalized(desc)
    _refuse(desc)
    return _plain.quantize_weights(desc, weights, ranges, QuantizedMixedNetModel, 1 if desc["pool"] else desc["t_final"])


# ---------------------------------------------------------------------------------------- calibration / public API

def _description(model, stride=None):
    """the stream-mode description of a trained MixedNet ``model``; refuses attention and first_conv_filters = 0"""
    from .layout import _flag
    from .streaming import mixednet_stream_description
    refuse_inception(model)
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
