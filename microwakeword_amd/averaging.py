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

The BatchNorm moving statistics are not trainable and are NOT averaged: they were accumulated under the raw iterates.  The
averaged model gets statistics of its own by re-estimation (``mww_bn_reestimate_*``, ``csrc/kernels_bnre.hip.h``):

State: ``ema_bn[S]`` in float32, laid out and indexed like ``Engine.get_bn_state()``, and a validity flag.  A pass over
``K >= 1`` batches of exactly ``b`` windows:

  * batch ``k``: the forward of ``Engine.forward(b, training=True, update_metrics=False)`` - batch statistics, moving
    statistics untouched, no loss, no metrics, no dropout - reading the AVERAGE (under ``weight_qat``: ``fake_quant(average)``,
    as an ``ema_forward`` evaluation reads it).  For every statistic slot ``s`` - a BN channel, a (channel, sub-band) slot of
    a SubSpectralNormalization - ``mean_k[s]`` / ``var_k[s]`` are the float32 batch mean and biased batch variance that
    forward normalised with, bit for bit (the engine re-derives them from the sums its own fold consumed, with that fold's
    expressions and summation order; the published ``rstd`` is another float).  They are accumulated in float64, in batch
    order: ``M[s] += float64(mean_k[s])``, ``V[s] += float64(var_k[s])``;
  * commit: ``ema_bn[o_mm + s] = float32(M[s] / float64(K))``, likewise the variance; the flag is set.

The master's ``bn_state`` is never written; there are no atomics, so two passes over the same batches write the same bytes;
nothing random is drawn.  While the flag is set, an ``ema_forward`` evaluation folds ``ema_bn`` instead of the master's
moving statistics.  Whatever changes what such an evaluation reads - an update of the average, ``set_ema_state``, installing
or removing the average, the ``weight_qat`` option or map - clears the flag, and evaluations read the master's moving
statistics again.  ``bn_reestimate`` below restates the accumulation and the commit.

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


def bn_reestimate(means, variances):
    """the commit of a re-estimation pass: ``means`` / ``variances`` [K, n] float32, the batch statistics of batches
    0 .. K - 1 -> (mean [n], variance [n]) float32: float64 sums in batch order, one division by K, one rounding"""
    out = []
    for rows in (means, variances):
        rows = np.asarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[0] < 1:
            raise ValueError("bn_reestimate takes [K, n] arrays with K >= 1")
        acc = np.zeros(rows.shape[1], np.float64)
        for row in rows:
            acc = acc + row.astype(np.float64)
        out.append((acc / np.float64(rows.shape[0])).astype(np.float32))
    return out[0], out[1]


def bn_rank_mean(states):
    """data-parallel training with rank-local BatchNorm: the ranks' ``ema_bn`` vectors [W, S] -> the one every rank installs,
    ``float32(sum_r float64(ema_bn_r) / W)`` (``parallel.DataParallel.average_ema_bn_state``)"""
    states = np.asarray(states, np.float32)
    return (states.astype(np.float64).sum(0) / np.float64(states.shape[0])).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the training-loop option
CONFIG_KEY = "weight_averaging"


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def parse_config(config: dict) -> Optional[dict]:
    """``weight_averaging`` of a training configuration -> {"decay": float, "first_step": int, "every_steps": int} or None
    when the key is absent.  ``decay`` and ``first_step`` are required.  With the optional mapping ``bn_reestimate:
    {samples: N, seed: 0}`` the result also holds ``"bn_reestimate": {"samples": int, "seed": int}`` (``samples`` required,
    >= 1).  Unknown keys and bad values are ValueErrors that name the key."""
    if CONFIG_KEY not in config or config[CONFIG_KEY] is None:
        return None
    opt = config[CONFIG_KEY]
    if not isinstance(opt, dict):
        raise ValueError("%s must be a mapping with the keys decay, first_step and (optionally) every_steps" % CONFIG_KEY)
    unknown = sorted(set(map(str, opt)) - {"decay", "first_step", "every_steps", "bn_reestimate"})
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
    out = {"decay": float(decay), "first_step": int(first), "every_steps": int(every)}
    if opt.get("bn_reestimate") is not None:
        bn = opt["bn_reestimate"]
        name = CONFIG_KEY + ".bn_reestimate"
        if not isinstance(bn, dict):
            raise ValueError("%s must be a mapping with the keys samples and (optionally) seed" % name)
        unknown = sorted(set(map(str, bn)) - {"samples", "seed"})
        if unknown:
            raise ValueError("%s: unknown key %s" % (name, ", ".join(unknown)))
        if "samples" not in bn:
            raise ValueError("%s.samples is required" % name)
        if not _integer(bn["samples"]) or int(bn["samples"]) < 1:
            raise ValueError("%s.samples must be an integer >= 1, got %r" % (name, bn["samples"]))
        seed = bn.get("seed", 0)
        if not _integer(seed) or int(seed) < 0:
            raise ValueError("%s.seed must be an integer >= 0, got %r" % (name, seed))
        out["bn_reestimate"] = {"samples": int(bn["samples"]), "seed": int(seed)}
    return out


def bn_reestimate_windows(settings, data_processor, features_length, batch) -> Optional[np.ndarray]:
    """The windows of the loop's re-estimation passes, drawn once: ``draw_seeded_windows(samples, T, seed)`` (resident training
    rows, mined providers skipped, no RNG stream moves), cut down to whole batches of ``batch``.  None without the key; fewer
    than one batch is a ValueError."""
    bn = (settings or {}).get("bn_reestimate")
    if bn is None:
        return None
    if not hasattr(data_processor, "draw_seeded_windows"):
        raise ValueError("%s.bn_reestimate needs this package's FeatureHandler (the passes read resident training rows)" % CONFIG_KEY)
    whole = (bn["samples"] // int(batch)) * int(batch)
    if whole < 1:
        raise ValueError("%s.bn_reestimate.samples = %d is less than one batch of %d windows" % (CONFIG_KEY, bn["samples"], int(batch)))
    return data_processor.draw_seeded_windows(bn["samples"], int(features_length), bn["seed"])[:whole]
