"""Weight averaging: the exponential moving average (EMA) of the trainable parameters the engine keeps on the device
(``mww_set_weight_ema`` in ``include/mww.h``, ``csrc/kernels_ema.hip.h``), stated once, with its NumPy restatement.

State: ``ema[P]`` in float32 over the engine's flat parameter vector - laid out and indexed like ``Engine.get_params()`` -
and an integer count ``updates``.  One update, given the master ``w``, a decay ``d`` in (0, 1) and ``om = 1.0 - d`` formed
in double:

  * ``updates == 0``:  ``ema[i] = w[i]``, a bit copy;
  * otherwise:         ``ema[i] = float32(float64(ema[i]) + om * (float64(w[i]) - float64(ema[i])))`` - three float64
    operations (subtract, multiply, add; not contracted into a fused multiply-add), then one rounding to float32.

The update follows every Adam update after which the optimizer step count is a multiple of ``every_steps``.  Nothing is
screened: a non-finite master propagates into the average, so a diverged run looks diverged.

The BatchNorm moving statistics are not trainable and are NOT averaged: an evaluation on the average reads the current
moving statistics, which were accumulated under the raw iterates.  This is the one known mismatch.

Keras carries the same idea as ``Adam(use_ema=True, ema_momentum=...)``; the reference leaves it off.  That ``decay``
corresponds to ``ema_momentum`` is our reading of the Keras documentation, not something a test pins.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def ema_update(ema: Optional[np.ndarray], w: np.ndarray, decay: float, updates: int) -> np.ndarray:
    """the average after one more update with master ``w`` (``updates`` = the number of updates ``ema`` has taken so far)"""
    w = np.asarray(w, np.float32)
    if updates == 0:
        return w.copy()
    om = 1.0 - float(decay)   # Python floats are doubles
    e = np.asarray(ema, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = w.astype(np.float64) - e
        t = om * d
        return (e + t).astype(np.float32)


def ema_fold(masters, decay: float, every_steps: int = 1, first_opt_step: int = 1, ema=None, updates: int = 0):
    """``ema_update`` folded over the masters read after consecutive optimizer steps ``first_opt_step, first_opt_step + 1, ..``:
    -> (ema, updates) behind the last of them"""
    for k, w in enumerate(masters):
        if (first_opt_step + k) % every_steps == 0:
            ema = ema_update(ema, w, decay, updates)
            updates += 1
    return ema, updates


# ---------------------------------------------------------------------------------------------- the training-loop option
CONFIG_KEY = "weight_averaging"


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def parse_config(config: dict) -> Optional[dict]:
    """``weight_averaging`` of a training configuration -> {"decay": float, "first_step": int, "every_steps": int} or None
    when the key is absent.  ``decay`` and ``first_step`` are required.  Unknown keys and bad values are ValueErrors that
    name the key."""
    if CONFIG_KEY not in config or config[CONFIG_KEY] is None:
        return None
    opt = config[CONFIG_KEY]
    if not isinstance(opt, dict):
        raise ValueError("%s must be a mapping with the keys decay, first_step and (optionally) every_steps" % CONFIG_KEY)
    unknown = sorted(set(map(str, opt)) - {"decay", "first_step", "every_steps"})
    if unknown:
        raise ValueError("%s: unknown key %s" % (CONFIG_KEY, ", ".join(unknown)))
    for key in ("decay", "first_step"):
        if key not in opt:
            raise ValueError("%s.%s is required" % (CONFIG_KEY, key))
    decay = opt["decay"]
    if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)) or not 0.0 < float(decay) < 1.0:
        raise ValueError("%s.decay must be a number in (0, 1), got %r" % (CONFIG_KEY, decay))
    first = opt["first_step"]
    if not _integer(first) or int(first) < 0:
        raise ValueError("%s.first_step must be an integer >= 0, got %r" % (CONFIG_KEY, first))
    every = opt.get("every_steps", 1)
    if not _integer(every) or int(every) < 1:
        raise ValueError("%s.every_steps must be an integer >= 1, got %r" % (CONFIG_KEY, every))
    return {"decay": float(decay), "first_step": int(first), "every_steps": int(every)}
