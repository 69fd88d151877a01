"""Hard-negative mining on the device: the places where a trained model fires on negative audio, fed back as training
samples without copying a row.

    clips, report = mining.mine_hard_negatives(streaming_model, data_processor, cutoff=0.5)
    data_processor.add_mined_provider(clips, sampling_weight=2.0)        # then train on

``mine_hard_negatives`` scores every negative track of ``mode`` in one native call (``StreamingModel.predict_tracks``),
locates the detections on the device (``mww_stream_detections``) and turns each into a slice of the store the track already
lives in (``streaming.detection_clips``); ``FeatureHandler.add_mined_provider`` makes those slices a training provider that
aliases the resident rows.  Nothing here draws from Python's or numpy's random generators.  Mining under data parallelism
is out of scope (``add_mined_provider`` refuses a sharded handler).

``mine_hard_negatives_on_device`` returns the same ``(clips, report)`` with the selection and the clip arithmetic done on the
device (``mww_stream_mine``): only the kept clips cross to the host.  ``train.train`` calls it at evaluation boundaries when the
configuration has a ``hard_negative_mining`` mapping (``MiningRounds``)."""
from __future__ import annotations

import logging
import os

import numpy as np

from . import streaming


def mine_hard_negatives(streaming_model, data_processor, cutoff, mode="training", max_new=None, before=0, after=0,
                        sliding_window_length=5, ignore_slices_after_accept=25):
    """Runs ``streaming_model`` over the label-0 tracks of ``mode`` and returns ``(clips, report)``: ``clips`` are
    ``mww_window`` descriptors of the rows behind every detection at ``cutoff`` (``before`` / ``after`` extra rows of
    context; with 0 / 0 exactly the window that fired), in (track, index) order; ``max_new`` keeps the highest moving
    averages, ties to the earlier (track, index), sorted on the host.  ``report``: count, detections (before ``max_new``),
    hours scanned (test.py:117), per-provider counts, cutoff, mode.  A stream-mode model is reset first, so a repeated call
    gives the same clips.  The default mode is "training": clips mined from a ``testing*`` set put evaluation audio into
    training - allowed, with a warning."""
    if mode.startswith("testing"):
        logging.warning("mining hard negatives from %r: training on them contaminates the evaluation on that set", mode)
    sm = streaming_model
    windows, _ = data_processor.track_windows(mode, sm.frames, only_label=0.0)
    provider_of = np.concatenate([np.full(len(p.feature_sets[mode]) * len(p.fixed_right_cutoffs), i, np.int64)
                                  for i, p in enumerate(data_processor.feature_providers) if p.label == 0.0] + [np.zeros(0, np.int64)])
    report = dict(cutoff=float(cutoff), mode=mode, tracks=int(windows.size), detections=0, count=0, hours=0.0, per_provider={})
    if not windows.size:
        return windows[:0], report
    sm.reset()
    offsets, _ = sm.predict_tracks(data_processor, mode, only_label=0.0)   # the same windows, in one native call
    kind = np.zeros(windows.size, np.int32)
    events, _, _, _ = sm.detections(offsets, kind, cutoff, sliding_window_length, ignore_slices_after_accept)
    lengths = np.maximum(np.diff(offsets) - sliding_window_length + 1, 0)
    step_s = data_processor.feature_providers[0].step
    report["hours"] = streaming.track_hours(lengths, sm.stride, step_s)
    report["detections"] = int(events.size)
    if max_new is not None and events.size > int(max_new):
        best = np.argsort(-events["average"].astype(np.float64), kind="stable")[:int(max_new)]   # stable: ties keep (track, index) order
        events = events[np.sort(best)]
    clips, kept = streaming.detection_clips(windows, events, sm.frames, sm.stride, sm.mode, sliding_window_length, before, after,
                                            return_kept=True)
    report["count"] = int(clips.size)
    who = provider_of[events["track"][kept]]
    report["per_provider"] = {int(i): int(np.count_nonzero(who == i)) for i in np.unique(who)}
    return clips, report


def mine_hard_negatives_on_device(streaming_model, data_processor, cutoff, mode="training", max_new=None, before=0, after=0,
                                  sliding_window_length=5, ignore_slices_after_accept=25):
    """``mine_hard_negatives`` with the selection of the ``max_new`` highest moving averages and the clip arithmetic on the
    device (``StreamingModel.mine``): the same ``(clips, report)``, key for key and byte for byte, ``per_provider`` counted
    from the kept events; the host reads the kept clips and the per-track counts, never the event list."""
    if mode.startswith("testing"):
        logging.warning("mining hard negatives from %r: training on them contaminates the evaluation on that set", mode)
    sm = streaming_model
    windows, _ = data_processor.track_windows(mode, sm.frames, only_label=0.0)
    provider_of = np.concatenate([np.full(len(p.feature_sets[mode]) * len(p.fixed_right_cutoffs), i, np.int64)
                                  for i, p in enumerate(data_processor.feature_providers) if p.label == 0.0] + [np.zeros(0, np.int64)])
    report = dict(cutoff=float(cutoff), mode=mode, tracks=int(windows.size), detections=0, count=0, hours=0.0, per_provider={})
    if not windows.size:
        return windows[:0], report
    sm.reset()
    offsets, _ = sm.predict_tracks(data_processor, mode, only_label=0.0)
    clips, events, detections, _ = sm.mine(windows, offsets, cutoff, sliding_window_length, ignore_slices_after_accept, before, after,
                                           None if max_new is None else int(max_new))
    lengths = np.maximum(np.diff(offsets) - sliding_window_length + 1, 0)
    report["hours"] = streaming.track_hours(lengths, sm.stride, data_processor.feature_providers[0].step)
    report["detections"] = int(detections)
    report["count"] = int(clips.size)
    who = provider_of[events["track"]]
    report["per_provider"] = {int(i): int(np.count_nonzero(who == i)) for i in np.unique(who)}
    return clips, report


# ---- the training-loop option (train.train)
KEY = "hard_negative_mining"
DEFAULTS = dict(every_evals=1, first_step=0, max_new=2000, max_total=None, sampling_weight=1.0, penalty_weight=1.0, mode="stream",
                sliding_window_length=5, ignore_slices_after_accept=25, before=0, after=0)


def mining_config(config, world=1):
    """The ``hard_negative_mining`` mapping of a training configuration with its defaults filled in, or None without the
    key.  Unknown keys, out-of-range values and a world size above 1 are ``ValueError``s that name the key."""
    given = config.get(KEY)
    if given is None:
        return None
    if not isinstance(given, dict):
        raise ValueError("%s must be a mapping (cutoff, every_evals, ...)" % KEY)
    from .quantize import LOOP_DEFAULTS, loop_settings
    unknown = sorted(set(given) - set(DEFAULTS) - set(LOOP_DEFAULTS) - {"cutoff"}, key=str)
    if unknown:
        raise ValueError("%s: unknown key(s) %s; known: cutoff, %s" % (KEY, ", ".join(map(str, unknown)),
                                                                       ", ".join(list(DEFAULTS) + list(LOOP_DEFAULTS))))
    if "cutoff" not in given:
        raise ValueError("%s: cutoff is required" % KEY)
    m = loop_settings(KEY, dict(DEFAULTS, **given))
    try:
        m["cutoff"] = float(m["cutoff"])
        for k in ("every_evals", "first_step", "max_new", "sliding_window_length", "ignore_slices_after_accept", "before", "after"):
            m[k] = int(m[k])
        m["max_total"] = 5 * m["max_new"] if m["max_total"] is None else int(m["max_total"])
        m["sampling_weight"], m["penalty_weight"] = float(m["sampling_weight"]), float(m["penalty_weight"])
    except (TypeError, ValueError):
        raise ValueError("%s: cutoff and the weights are numbers, the other values integers (mode: stream / non_stream)" % KEY) from None
    bad = [k for k, ok in (("cutoff", m["cutoff"] == m["cutoff"]), ("every_evals", m["every_evals"] >= 1), ("first_step", m["first_step"] >= 0),
                           ("max_new", m["max_new"] >= 1), ("max_total", m["max_total"] >= m["max_new"]),
                           ("sampling_weight", m["sampling_weight"] >= 0), ("penalty_weight", m["penalty_weight"] >= 0),
                           ("mode", m["mode"] in ("stream", "non_stream")), ("sliding_window_length", m["sliding_window_length"] >= 1),
                           ("ignore_slices_after_accept", m["ignore_slices_after_accept"] >= 0), ("before", m["before"] >= 0),
                           ("after", m["after"] >= 0)) if not ok]
    if bad:
        raise ValueError("%s: %s out of range (every_evals, max_new, sliding_window_length >= 1; max_total >= max_new; first_step, "
                         "the weights, ignore_slices_after_accept, before, after >= 0; mode stream or non_stream)" % (KEY, ", ".join(bad)))
    if int(world) > 1:
        raise ValueError("%s is not available under data parallelism (world size %d): a sharded handler refuses mined providers"
                         % (KEY, int(world)))
    return m


def merge_clips(old, old_round, new, new_round, max_total):
    """The accumulated list after a round: clips are keyed by (store, src_elem, rows); old clips that were not mined again
    keep their order, this round's follow in the order given (a clip mined again moves to the end; one that the round names
    twice stays where it is named first), and a list longer than ``max_total`` loses clips from the front."""
    key = lambda c: (int(c["store"]), int(c["src_elem"]), int(c["copy_rows"]))   # noqa: E731
    seen, first = set(), []
    for j, c in enumerate(new):
        if key(c) not in seen:
            seen.add(key(c))
            first.append(j)
    keep = [j for j, c in enumerate(old) if key(c) not in seen]
    clips = np.concatenate([old[keep], new[first]])
    rounds = np.concatenate([np.asarray(old_round, np.int64)[keep], np.full(len(first), int(new_round), np.int64)])
    drop = max(clips.size - int(max_total), 0)
    return clips[drop:], rounds[drop:]


class MiningRounds:
    """What ``train.train`` does with a ``hard_negative_mining`` mapping: at the evaluation boundaries that are due, one
    ``mine_hard_negatives_on_device`` over the label-0 ``"training"`` tracks with the model's current weights, merged into
    one mined provider of the handler.  A round draws nothing from Python's or numpy's generators.  With ``quantized`` a round
    mines with the int8 model of those weights (``quantize.LoopQuantizer``; ``quantizer``: the one a quantized
    ``streaming_validation`` already made, to be shared), through the same ``mine_hard_negatives_on_device``."""

    FILE = "mined_clips.npz"

    def __init__(self, settings, model, data_processor, config, writer=None, quantizer=None):
        from . import native
        from .quantize import loop_quantizer
        if getattr(data_processor, "engine", None) is not getattr(model, "engine", object()) or not hasattr(data_processor, "add_mined_provider"):
            raise ValueError("%s needs this package's Model and FeatureHandler on one engine: the clips alias rows resident "
                             "in the model's context" % KEY)
        self.m, self.model, self.fh, self.writer = settings, model, data_processor, writer
        self.stride = int(config["stride"])
        self.quantizer = loop_quantizer(KEY, settings, model, data_processor, config, quantizer)   # its refusals, before any file
        self.path = os.path.join(config["train_dir"], self.FILE) if writer is not None else None
        self.sm = None
        self.provider = None
        self.boundaries = 0
        self.rounds = 0
        self.clips, self.clip_round = np.zeros(0, native.WINDOW_DTYPE), np.zeros(0, np.int64)
        if self.path and os.path.isfile(self.path):
            self._restore()

    def _stores(self):
        """store id -> (provider index, dtype key, elements) of the providers that own rows"""
        return {int(sid): (i, key, int(p.flat[key].size)) for i, p in enumerate(self.fh.feature_providers)
                if p is not self.provider and getattr(p, "flat", None) for key, sid in p.store_id.items()}

    def _restore(self):
        from . import native
        with np.load(self.path) as z:
            prov, keys, elem, rows, rnd = z["provider"], [str(k) for k in z["dtype_key"]], z["src_elem"], z["rows"], z["round"]
        sid = {(i, key): (s, size) for s, (i, key, size) in self._stores().items()}
        clips = np.zeros(len(prov), native.WINDOW_DTYPE)
        for j in range(len(prov)):
            where = sid.get((int(prov[j]), keys[j]))
            if where is None or rows[j] <= 0 or elem[j] < 0 or elem[j] % 40 or elem[j] + rows[j] * 40 > where[1]:
                logging.warning("%s: clip %d of %s does not lie inside a store of this run: starting with an empty list", KEY, j, self.path)
                return
            clips[j] = (where[0], 0, int(rows[j]), 0, int(elem[j]))
        self.clips, self.clip_round = clips, np.asarray(rnd, np.int64)
        self.rounds = int(self.clip_round.max()) if clips.size else 0
        if clips.size:
            self.provider = self.fh.add_mined_provider(clips, sampling_weight=self.m["sampling_weight"], penalty_weight=self.m["penalty_weight"])

    def _save(self):
        if not self.path:
            return
        stores = self._stores()
        np.savez(self.path, provider=np.array([stores[int(s)][0] for s in self.clips["store"]], np.int64),
                 dtype_key=np.array([stores[int(s)][1] for s in self.clips["store"]], dtype="U8"),
                 src_elem=self.clips["src_elem"].astype(np.int64), rows=self.clips["copy_rows"].astype(np.int64), round=self.clip_round)

    def due(self, step, is_last):
        """called once per evaluation boundary: whether a round runs at this one (never at the last step: nothing trains after it)"""
        self.boundaries += 1
        return not is_last and self.boundaries % self.m["every_evals"] == 0 and step >= self.m["first_step"]

    def round(self, step):
        from . import streaming
        m = self.m
        if self.quantizer is not None:   # the int8 model of the current weights (calibrated once per boundary, whoever asks)
            try:
                q = self.quantizer.at(step)
            except ValueError as e:
                raise ValueError("%s: quantized: %s" % (KEY, e)) from None
            if self.sm is not None:
                self.sm.native.close()
            self.sm = streaming.QuantizedStreamingModel(q, self.stride, m["mode"], context=self.model)
        else:
            if self.sm is None:
                self.sm = streaming.StreamingModel(self.model, self.stride, m["mode"])   # on the model's own context
            self.sm.set_weights(self.model.get_weights())
        own = [p for p in self.fh.feature_providers if p is not self.provider]   # the mined clips alias rows that are scanned anyway
        saved, self.fh.feature_providers = self.fh.feature_providers, own
        try:
            clips, report = mine_hard_negatives_on_device(self.sm, self.fh, m["cutoff"], "training", m["max_new"], m["before"], m["after"],
                                                          m["sliding_window_length"], m["ignore_slices_after_accept"])
        finally:
            self.fh.feature_providers = saved
        self.rounds += 1
        if clips.size:
            self.clips, self.clip_round = merge_clips(self.clips, self.clip_round, clips, self.rounds, m["max_total"])
            if self.provider is None:
                self.provider = self.fh.add_mined_provider(self.clips, sampling_weight=m["sampling_weight"], penalty_weight=m["penalty_weight"])
            else:
                self.fh.set_mined_clips(self.provider, self.clips)
            self._save()
        if self.writer is not None:
            hours = report["hours"]
            self.writer.scalars(step, detections=report["detections"], kept=report["count"], total=self.clips.size, hours=hours,
                                detections_per_hour=report["detections"] / hours if hours > 0 else 0.0)
        logging.getLogger("microwakeword_amd.train").info(
            "Step %d: mined %d hard negatives of %d detections in %.3f h; the mined provider holds %d clips", step, report["count"],
            report["detections"], report["hours"], self.clips.size)
        return report
