"""Sharpness-aware train steps (SAM) and global-norm gradient clipping: what the engine computes between the backward pass and
Adam (``mww_set_sharpness_aware`` / ``mww_set_grad_clip`` in ``include/mww.h``, ``csrc/kernels_sam.hip.h``), stated
once, with NumPy restatements.  The device follows them operation for operation; the tests compare bytes.

``g`` is the flat float32 gradient, laid out and indexed like ``Engine.get_grads()``; ``w`` the flat float32 master.

Sum of squares ``S = sumsq(g)``: 1024 lanes; lane ``j`` holds the float64 sum of ``float64(g[i]) * float64(g[i])`` over
``i = j, j + 1024, j + 2048, ...`` in ascending order, accumulated sequentially from 0.0, the multiply and the add two operations
(no fused multiply-add); then ``S = ((s_0 + s_1) + s_2) + ...`` in lane order.  No atomics: two calls give the same bytes.

Perturbation (a sharpness-aware step, radius ``rho > 0``): ``scale = rho / (sqrt(S) + 1e-12)`` in float64;
``e[i] = float32(scale * float64(g[i]))``; ``w'[i] = w[i] + e[i]``, one float32 add.  Every trainable parameter takes part; a
structurally masked tap has gradient 0 and does not move.  The step takes a second gradient at ``w'`` (same batch, same dropout
mask), puts the master back from a bit copy - never by subtracting ``e`` - and hands that second gradient to Adam at ``w``.

Clipping (threshold ``c > 0``, Keras ``global_clipnorm``): ``k = c / max(sqrt(S), c)`` in float64, where ``max(r, c)`` is ``r``
if ``r > c`` else ``c`` - so ``k`` is exactly 1.0 at or below the threshold (and for a NaN ``S``); ``g[i] = float32(k *
float64(g[i]))`` in place, which for ``k == 1.0`` leaves every bit of ``g`` as it was.

Nothing is screened: a non-finite gradient gives a non-finite ``S``, ``scale`` and ``w'``, and a diverged run looks diverged.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

LANES = 1024
EPS = 1e-12


def sumsq(g) -> float:
    """``S`` of the flat gradient ``g``, as a Python float (a double)"""
    g = np.asarray(g, np.float32).reshape(-1).astype(np.float64)
    n = g.size
    rows = -(-n // LANES) if n else 1
    sq = np.zeros(rows * LANES, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sq[:n] = g * g
        # lane j is column j; np.cumsum accumulates sequentially, in row (ascending i) order, unlike np.sum.  The padding adds
        # + 0.0 behind a lane's last element, which changes no bit of a sum of squares (never -0.0)
        lanes = np.cumsum(sq.reshape(rows, LANES), axis=0)[-1]
        return float(np.cumsum(lanes)[-1])


def perturb_scale(S: float, rho: float) -> float:
    r = math.sqrt(float(S))   # (correctly rounded; S is never negative; inf and NaN pass through)
    return float(rho) / (r + EPS)


def perturb(w, g, rho: float, S: Optional[float] = None) -> np.ndarray:
    """``w'`` of a sharpness-aware step"""
    w = np.asarray(w, np.float32).reshape(-1)
    g = np.asarray(g, np.float32).reshape(-1)
    scale = np.float64(perturb_scale(sumsq(g) if S is None else S, rho))
    with np.errstate(invalid="ignore", over="ignore"):
        e = (scale * g.astype(np.float64)).astype(np.float32)
        return w + e


def clip_factor(S: float, c: float) -> float:
    r = math.sqrt(float(S))
    c = float(c)
    return c / (r if r > c else c)


def clip(g, c: float, S: Optional[float] = None) -> np.ndarray:
    """the gradient Adam consumes under global-norm clipping at ``c``"""
    g = np.asarray(g, np.float32).reshape(-1)
    k = np.float64(clip_factor(sumsq(g) if S is None else S, c))
    with np.errstate(invalid="ignore", over="ignore"):
        return (k * g.astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the training-loop options
SAM_KEY = "sharpness_aware"
CLIP_KEY = "gradient_clipping"


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _positive(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(float(v)) and float(v) > 0.0


def _mapping(config, key, allowed):
    if key not in config or config[key] is None:
        return None
    opt = config[key]
    if not isinstance(opt, dict):
        raise ValueError("%s must be a mapping with the keys %s" % (key, ", ".join(allowed)))
    unknown = sorted(set(map(str, opt)) - set(allowed))
    if unknown:
        raise ValueError("%s: unknown key %s" % (key, ", ".join(unknown)))
    return opt


def parse_sam_config(config: dict) -> Optional[dict]:
    """``sharpness_aware`` of a training configuration -> {"rho": float, "first_step": int} or None when the key is absent.
    ``rho`` is required, finite and > 0; ``first_step`` (default 0) an integer >= 0.  Unknown keys and bad values are
    ValueErrors that name the key."""
    opt = _mapping(config, SAM_KEY, ("rho", "first_step"))
    if opt is None:
        return None
    if "rho" not in opt:
        raise ValueError("%s.rho is required" % SAM_KEY)
    if not _positive(opt["rho"]):
        raise ValueError("%s.rho must be a finite number > 0, got %r" % (SAM_KEY, opt["rho"]))
    first = opt.get("first_step", 0)
    if not _integer(first) or int(first) < 0:
        raise ValueError("%s.first_step must be an integer >= 0, got %r" % (SAM_KEY, first))
    return {"rho": float(opt["rho"]), "first_step": int(first)}


def parse_clip_config(config: dict) -> Optional[dict]:
    """``gradient_clipping`` of a training configuration -> {"global_norm": float} or None when the key is absent"""
    opt = _mapping(config, CLIP_KEY, ("global_norm",))
    if opt is None:
        return None
    if "global_norm" not in opt:
        raise ValueError("%s.global_norm is required" % CLIP_KEY)
    if not _positive(opt["global_norm"]):
        raise ValueError("%s.global_norm must be a finite number > 0, got %r" % (CLIP_KEY, opt["global_norm"]))
    return {"global_norm": float(opt["global_norm"])}


def parse_config(config: dict, world: int = 1):
    """both mappings -> (sam, clip); either with more than one rank is refused (single-device for now)"""
    sam, clp = parse_sam_config(config), parse_clip_config(config)
    if world > 1:
        for key, got in ((SAM_KEY, sam), (CLIP_KEY, clp)):
            if got is not None:
                raise ValueError("%s is single-device for now: it cannot run with %d ranks (the gradient norm would have to be taken "
                                 "behind the exchange)" % (key, world))
    return sam, clp
