"""Hard-negative mining on the device: the places where a trained model fires on negative audio, fed back as training
samples without copying a row.

    clips, report = mining.mine_hard_negatives(streaming_model, data_processor, cutoff=0.5)
    data_processor.add_mined_provider(clips, sampling_weight=2.0)        # then train on

``mine_hard_negatives`` scores every negative track of ``mode`` in one native call (``StreamingModel.predict_tracks``),
locates the detections on the device (``mww_stream_detections``) and turns each into a slice of the store the track already
lives in (``streaming.detection_clips``); ``FeatureHandler.add_mined_provider`` makes those slices a training provider that
aliases the resident rows.  Nothing here draws from Python's or numpy's random generators.  Mining under data parallelism
is out of scope (``add_mined_provider`` refuses a sharded handler)."""
from __future__ import annotations

import logging

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
