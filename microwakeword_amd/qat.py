"""Weight-only quantization-aware training: which native parameters form a weight channel, and the NumPy restatement of
the shadow the engine's ``weight_qat`` option puts in front of the forward / backward kernels (``include/mww.h``).

The grid is the one the int8 streaming family ships: ``quantize.weight_params`` (symmetric, narrow range, one scale per
output channel, ties away from zero).  The kernels are the 4-D Keras variables and the dense kernel; their channel axes
are the ones the quantizers hand to ``weight_params``:

  * ``[k, 1, Cin, Cout]``      axis 3   ``quantize.py:361`` (conv1 as ``[k * 40, C1]``, axis 1), ``quantize.py:212`` (a folded
                                        1x1 ``[Ci, Co]``, axis 1), ``quantize_graph.py:165`` (``[k, cin, cout]``, axis 2)
  * depthwise ``[k, 1, C, 1]`` axis 2   ``quantize.py:372`` (the fused tap table ``[K, C]``, axis 1: a group's taps and the
                                        structural zeros above them share the column's scale)
  * dense ``[n, 1]``           axis 1   ``quantize.py:222``

Per-channel symmetric quantization does not change under a positive per-channel rescaling, so folding BatchNorm into a 1x1
kernel (``quantize.fold_bn``) leaves a channel's grid where it is up to float rounding at ties and the sign of gamma: the
shadow is, channel by channel, the set of values the shipped int8 kernel can represent.  Activations are not fake-quantized.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .quantize import weight_params

_DEPTHWISE = re.compile(r"\.dw\d+\.kernel$")


def kernel_axis(name: str, shape) -> Optional[int]:
    """the channel axis of Keras variable ``name`` if it is a quantized kernel, else None"""
    if not name.endswith(".kernel"):
        return None
    if len(shape) == 4:
        return 2 if _DEPTHWISE.search(name) else 3
    if name == "dense.kernel" and len(shape) == 2:
        return 1
    return None


def _layout(model_or_layout):
    return getattr(model_or_layout, "layout", model_or_layout)


def channel_map(layout) -> Tuple[np.ndarray, np.ndarray]:
    """(chan_start int32 [C + 1], chan_elem int32 [n]) for ``mww_set_weight_qat``: channel c owns the native parameter
    indices ``chan_elem[chan_start[c]:chan_start[c + 1]]``.  Channels follow the Keras variables in ``keras_vars`` order,
    then the channel index.  The native position of every Keras element comes from packing arrays of element ids through
    the layout's own ``pack`` (ids stay below 2^24, exact in float32), so masked MixConv taps - which no Keras element
    reaches - stay outside every channel, like biases and BN variables."""
    layout = _layout(layout)
    ids, nxt = [], 1
    for _, shape, _ in layout.keras_vars:
        n = int(np.prod(shape))
        ids.append(np.arange(nxt, nxt + n, dtype=np.int64).reshape(shape))
        nxt += n
    if nxt >= 1 << 24:
        raise ValueError("model too large for the id-packing channel map (%d variables' elements)" % nxt)
    packed = layout.pack([a.astype(np.float32) for a in ids])[0].astype(np.int64)
    position = np.full(nxt, -1, np.int64)
    position[packed[packed > 0]] = np.nonzero(packed > 0)[0]
    starts, elems, at = [0], [], 0
    for (name, shape, kind), a in zip(layout.keras_vars, ids):
        axis = kernel_axis(name, shape) if kind == "param" else None
        if axis is None:
            continue
        rows = position[np.moveaxis(a, axis, 0).reshape(shape[axis], -1)]
        if (rows < 0).any():
            raise ValueError("kernel %s has elements without a native position" % name)
        for r in rows:
            elems.append(r)
            at += r.size
            starts.append(at)
    return np.asarray(starts, np.int32), (np.concatenate(elems) if elems else np.zeros(0, np.int64)).astype(np.int32)


def fake_quant_weights(model_or_layout, weights: Sequence[np.ndarray]) -> List[np.ndarray]:
    """The Keras-order weight list with every kernel on its int8 grid: per kernel ``quantize.weight_params`` along its
    channel axis, then ``q.astype(float32) * scale`` (one float32 multiply); everything else unchanged.  A channel whose
    largest magnitude is not finite is left as it is (the engine copies it through)."""
    layout = _layout(model_or_layout)
    out = []
    for (name, shape, kind), w in zip(layout.keras_vars, weights):
        w = np.asarray(w, np.float32)
        axis = kernel_axis(name, shape) if kind == "param" else None
        if axis is None or w.size == 0:
            out.append(w.copy())
            continue
        with np.errstate(all="ignore"):
            q, scale = weight_params(w, axis)
            bshape = [1] * w.ndim
            bshape[axis] = -1
            fq = q.astype(np.float32) * scale.reshape(bshape)
            red = tuple(i for i in range(w.ndim) if i != axis)
            bad = ~np.isfinite(np.abs(w.astype(np.float64)).max(axis=red))
        out.append(np.where(bad.reshape(bshape), w, fq).astype(np.float32))
    return out


def forward_params_reference(layout, params: np.ndarray, state: Optional[np.ndarray] = None) -> np.ndarray:
    """what the engine's shadow holds for the native parameter vector ``params``: the restatement above on every channel
    element, ``params`` itself everywhere else"""
    layout = _layout(layout)
    params = np.asarray(params, np.float32).reshape(-1)
    state = np.zeros(layout.n_state, np.float32) if state is None else state
    fq = layout.pack(fake_quant_weights(layout, layout.unpack(params, state)))[0]
    out = params.copy()
    _, elem = channel_map(layout)
    out[elem] = fq[elem]
    return out


# ---------------------------------------------------------------------------------------------- the training-loop option
CONFIG_KEY = "weight_quantization_aware"


def parse_config(config: dict) -> Optional[dict]:
    """``weight_quantization_aware`` of a training configuration -> {"first_step": int} or None when the key is absent.
    Unknown keys and bad values are ValueErrors that name the key."""
    if CONFIG_KEY not in config or config[CONFIG_KEY] is None:
        return None
    opt = config[CONFIG_KEY]
    if not isinstance(opt, dict):
        raise ValueError("%s must be a mapping with the key first_step" % CONFIG_KEY)
    unknown = sorted(set(opt) - {"first_step"})
    if unknown:
        raise ValueError("%s: unknown key %s" % (CONFIG_KEY, ", ".join(map(str, unknown))))
    first = opt.get("first_step", 0)
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or int(first) < 0:
        raise ValueError("%s.first_step must be an integer >= 0, got %r" % (CONFIG_KEY, first))
    return {"first_step": int(first)}
