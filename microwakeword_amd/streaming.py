"""Streaming inference and the FAPH / FRR evaluation of a trained MixedNet or Inception model on the MI355X - the step after training that the
reference runs with its ``--test_*`` flags (microwakeword/model_train_eval.py:131-272 ``evaluate_model``):

  * ``StreamingModel``            the model the reference converts with ``utils.convert_model_saved`` and runs through
                                  ``inference.Model`` (inference.py:82-125 ``predict_spectrogram``), as a native
                                  ``mww_stream`` (csrc/tu_stream.hip; Inception: csrc/tu_stream_graph.hip): ``mode="stream"`` is
                                  Modes.STREAM_INTERNAL_STATE_INFERENCE (``--test_tflite_streaming``), ``mode="non_stream"``
                                  the non-streaming model on every ``stride``-th window (``--test_tflite_nonstreaming``)
  * ``false_accepts_per_hour``    test.py:94-137 ``compute_false_accepts_per_hour``
  * ``roc_curve``                 test.py:140-204 ``generate_roc_curve`` (restated bug for bug: ``y1`` is read at
                                  ``index - 1`` and the interpolation uses the literal 2.0)
  * ``streaming_model_roc``       test.py:293-403 ``tflite_streaming_model_roc``
  * ``model_accuracy``            test.py:207-290 ``tf_model_accuracy`` (``--test_tf_nonstreaming``)

The MixedNet descriptions (``stream_description``, ``mixednet_stream_description``) read the flag set through
``layout.block_lists`` / ``layout.MixedNetTopology`` - the one topology walk - and add only their own refusals.

State carry-over, by our reading of test.py:321-324,355-365: the interpreter is created once and never reset, so the rings
carry over from the ambient tracks (in ``get_data`` order) to the positive tracks of the test set (negatives are skipped
without being fed).  ``streaming_model_roc`` reproduces exactly that.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np

from . import native
from .layout import FEATURE_BINS, InceptionLayout, MixedNetTopology, _flag, block_lists, parse

SCALE_U16 = np.float32(0.0390625)
CUTOFFS = np.arange(0, 1.01, 0.01)   # test.py:331
OP_WINDOWS = tuple(range(1, 11))     # sliding-window sizes of the operating-point grid (the reference evaluates 5 alone)


def stream_description(flags, t_final: int, frames: int, stride: int, mode: str) -> dict:
    """The ``mww_stream_desc`` of a MixedNet flag set (mixednet.py:307-386).  Topologies outside the streaming kernel raise
    NotImplementedError naming the flag."""
    if mode not in native.STREAM_MODES:
        raise ValueError("mode must be 'stream' or 'non_stream'")
    pf, rep, ksz, res = block_lists(flags)
    unsupported = []
    if int(_flag(flags, "first_conv_filters")) <= 0:
        unsupported.append("first_conv_filters = 0")
    if any(res):
        unsupported.append("residual_connection")
    if t_final > 1 and _flag(flags, "spatial_attention"):
        unsupported.append("spatial_attention")
    if t_final > 1 and _flag(flags, "pooled"):
        unsupported.append("pooled")
    if unsupported:
        raise NotImplementedError("streaming evaluation does not cover MixedNet with " + ", ".join(unsupported))
    if int(stride) != int(_flag(flags, "stride")):
        raise ValueError("the streaming stride (%d) must be the model's --stride (%d)" % (stride, _flag(flags, "stride")))
    return dict(conv1_filters=int(_flag(flags, "first_conv_filters")), conv1_kernel=int(_flag(flags, "first_conv_kernel_size")),
                stride=int(stride), blocks=list(zip(rep, ksz, pf)), t_final=int(t_final), frames=int(frames), mode=mode)


STREAM_ATTENTION_REASON = (
    "spatial_attention in stream mode: the reference's streaming clone replays the slice net[:, -T_a:] with its build-time bound "
    "next to a 4-tap Stream(Conv2D) that yields one frame, which by our reading gates the last T_f - 3 ring frames with the "
    "CURRENT attention value - not the non-streaming computation even when warm, and nothing available pins that reading")


def mixednet_variant_flags(flags) -> List[str]:
    """the flags of a MixedNet flag set that ask for a residual connection, a pooled head or spatial attention"""
    out = ["residual_connection"] if any(parse(_flag(flags, "residual_connection"))) else []
    return out + [name for name in ("pooled", "spatial_attention") if _flag(flags, name)]


def mixednet_stream_description(flags, frames: int, stride: int, mode: str) -> dict:
    """The ``mww_mixednet_stream_desc`` of any MixedNet flag set with a first convolution (mixednet.py:307-386): the keys of
    ``stream_description`` plus ``residual`` (0 / 1 per block), ``attention`` and ``pool`` (0 / "average" / "max").  ``t_final``
    is T_f, the frames of the final map BEFORE attention and pooling, derived from the flags and ``frames`` (a pooled
    layout's ``t_last`` is 1 whatever T_f is); with T_f = 1 the head flags do nothing and are dropped.  Raises
    NotImplementedError for ``first_conv_filters = 0`` and for spatial attention in stream mode, ValueError where the model
    itself cannot be built."""
    if mode not in native.STREAM_MODES:
        raise ValueError("mode must be 'stream' or 'non_stream'")
    topo = MixedNetTopology(flags, frames)
    if topo.conv1 is None:
        raise NotImplementedError("streaming evaluation does not cover MixedNet with first_conv_filters = 0")
    if int(stride) != topo.stride:
        raise ValueError("the streaming stride (%d) must be the model's --stride (%d)" % (stride, _flag(flags, "stride")))
    if topo.t_final < 1:   # the frame counts only fall along the layers
        raise ValueError("spectrogram of %d frames is too short for this network" % int(frames))
    attention, pool, _ = topo.head()
    if attention and mode == "stream":
        raise NotImplementedError("streaming evaluation does not cover MixedNet with " + STREAM_ATTENTION_REASON)
    return dict(conv1_filters=topo.conv1_filters, conv1_kernel=topo.conv1_kernel, stride=int(stride),
                blocks=list(zip(topo.repeats, topo.kernels, topo.filters)), t_final=topo.t_final, frames=int(frames), mode=mode,
                residual=[int(bool(r)) for r in topo.residual], attention=int(attention), pool={0: 0, 1: "average", 2: "max"}[pool])


def check_evaluation_topology(flags, frames: int, stride: int, modes: Sequence[str], int8: bool = False, int8_variants: bool = False):
    """What ``model_train_eval`` asks BEFORE it trains: raises NotImplementedError naming the flag when a requested
    streaming / non-streaming evaluation (``modes``) or the int8 one does not cover the MixedNet flag set.
    ``int8_variants`` (``--quantized_backend native_ext``): residual_connection and pooled pass the int8 check
    (quantize_mixednet.py); spatial attention and first_conv_filters = 0 are refused by the stream-mode description below."""
    if int8 and not int8_variants and mixednet_variant_flags(flags):
        raise NotImplementedError("the int8 quantized streaming evaluation does not cover MixedNet with "
                                  + ", ".join(mixednet_variant_flags(flags)) + " (--quantized_backend native_ext adds the restated "
                                  "int8 ADD, AVERAGE_POOL_2D and MAX_POOL_2D for residual_connection and pooled; int8 MUL is not restated)")
    for mode in list(modes) + (["stream"] if int8 and "stream" not in modes else []):   # the int8 model is a stream-mode model
        mixednet_stream_description(flags, frames, stride, mode)


def graph_stream_description(flags, frames: int, stride: int, mode: str) -> dict:
    """The description of a streaming Inception (inception.py:233-338) for ``native.GraphStream``: the un-fused op list in
    Keras layer-creation order, so ``get_weights()`` feeds it as it is.  Inception has no ``--stride``: one frame per
    step."""
    if mode not in native.STREAM_MODES:
        raise ValueError("mode must be 'stream' or 'non_stream'")
    if int(stride) != 1:
        raise ValueError("the streaming stride (%d) must be 1: an Inception model has no --stride" % int(stride))
    lay = InceptionLayout(flags, int(frames), fuse_heads=False)
    # the layout lists a block's three 1x1 branch heads first (b1, b2a, b3a, b2b, ...); Keras creates b1, b2a, b2b, b3a, ...
    order = sorted(range(len(lay.ops)), key=lambda o: lay.op_keras_index[o])
    at = {old: new for new, old in enumerate(order)}
    ops = [dict(lay.ops[o], src=[at[s] if s >= 0 else -1 for s in lay.ops[o]["src"]]) for o in order]
    assert all(s < i for i, op in enumerate(ops) for s in op["src"])
    return dict(conv_ops=ops, op_names=[lay.op_names[o] for o in order], frames=int(frames), stride=1, mode=mode)


class StreamingModel:
    """The streaming (``mode="stream"``) or non-streaming (``mode="non_stream"``) form of a trained MixedNet or Inception
    ``model`` (``microwakeword_amd.model.Model``, any kernel family; MixedNet on csrc/tu_stream.hip - with residual
    connections, a pooled head or, in non_stream mode, spatial attention on that kernel's <VAR> form -, Inception on
    csrc/tu_stream_graph.hip), sharing the model's context: its device, HIP stream and the
    feature stores a ``FeatureHandler`` uploaded there.  The weights are taken from ``model`` when this object is created
    (``set_weights`` takes new ones)."""

    def __init__(self, model, stride: int, mode: str = "stream"):
        self.model = model
        self.mode = mode
        self.stride = int(stride)
        lay = model.layout
        if not hasattr(lay, "t_last"):
            raise NotImplementedError("streaming evaluation covers MixedNet and Inception models")
        self.frames = int(lay.frames)   # input_feature_slices of the non-streaming model
        if isinstance(lay, InceptionLayout):
            self.desc = graph_stream_description(model.flags, lay.frames, stride, mode)
            self.native = native.GraphStream(model.engine, self.desc)
        elif mixednet_variant_flags(model.flags):   # residual / pooled / attention: T_f from the flags, not from lay.t_last
            self.desc = mixednet_stream_description(model.flags, lay.frames, stride, mode)
            self.native = native.Stream(model.engine, self.desc)
        else:
            self.desc = stream_description(model.flags, lay.t_last, lay.frames, stride, mode)
            self.native = native.Stream(model.engine, self.desc)
        self.set_weights(model.get_weights())

    def set_weights(self, weights: Sequence[np.ndarray]):
        self.native.set_weights(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in weights]))

    def reset(self):
        """Rings back to zeros (a freshly created interpreter)."""
        self.native.reset()

    def predict_spectrogram(self, spectrogram: np.ndarray) -> np.ndarray:
        """inference.py:82-125: uint16 rows are scaled by 0.0390625, float64 rows cast to float32; stream mode feeds frames
        [0, floor(L/s)*s) in chunks of s with the state carried from call to call, non-stream mode scores the windows ending
        at T, T + s, ... <= L.  Returns the probabilities as a float32 array (the reference returns a list of the same
        float32 values)."""
        x = np.asarray(spectrogram)
        if np.issubdtype(x.dtype, np.uint16):
            x = x.astype(np.float32) * SCALE_U16
        else:
            x = x.astype(np.float32)
        if x.ndim != 2 or x.shape[1] != FEATURE_BINS:
            raise ValueError("spectrogram must be [T, %d]" % FEATURE_BINS)
        self.native.run_host(x)
        return self.native.read()

    def predict_tracks(self, data_processor, mode: str, only_label: Optional[float] = None, features_length: Optional[int] = None):
        """Every track of ``data_processor.get_data(mode, ..., truncation_strategy="none")`` (or only those whose label is
        ``only_label``) in one native call over the resident stores.  Returns ``(offsets [n + 1], labels [n])``; the
        probabilities stay on the device (``read_probabilities``, ``metrics``)."""
        win, labels = data_processor.track_windows(mode, features_length or self.frames, only_label=only_label)
        offsets = self.native.run(win)
        return offsets, labels

    def read_probabilities(self) -> np.ndarray:
        return self.native.read()

    def metrics(self, offsets, kind, cutoffs=CUTOFFS, sliding_window_length=5, ignore_slices_after_accept=25):
        """Device-side detection metrics on the probabilities of the last call (see mww_stream_metrics)."""
        return self.native.metrics(offsets, kind, cutoffs, sliding_window_length, ignore_slices_after_accept, ignore_slices_after_accept)

    def detections(self, offsets, kind, cutoff, sliding_window_length=5, ignore_slices_after_accept=25):
        """Where the probabilities of the last call fire at ONE cutoff (mww_stream_detections; ``detection_positions`` is the
        host restatement): ``(events, track_count, best_index, score)`` - ``events`` a structured array (track, index,
        average) of the ambient (kind 0) tracks' false accepts in (track, index) order, ``best_index`` / ``score`` where a
        positive (kind 1) track reaches its maximum after the first ``ignore_slices_after_accept`` probabilities."""
        return self.native.detections(offsets, kind, cutoff, sliding_window_length, ignore_slices_after_accept, ignore_slices_after_accept)

    def mine(self, windows, offsets, cutoff, sliding_window_length=5, ignore_slices_after_accept=25, before=0, after=0, max_new=None):
        """The hard negatives of the tracks ``windows`` on the probabilities of the last call, selected and cut into clips on
        the device (mww_stream_mine): what ``detections`` on all-ambient tracks, a stable descending sort cut at ``max_new``
        and ``detection_clips`` give, without the event list crossing to the host.  -> (clips, events, detections before the
        selection, track_count)."""
        return self.native.mine(windows, offsets, cutoff, sliding_window_length, ignore_slices_after_accept, before, after, max_new)

    def operating_points(self, offsets, kind, windows=OP_WINDOWS, cutoffs=CUTOFFS, ignore_slices_after_accept=25):
        """``metrics`` at every sliding-window size of ``windows`` in one call (mww_stream_operating_points;
        ``operating_points_host`` is the host restatement): ``(counts [W, C], ma_len [W, n], score [W, n])``, row k what
        ``metrics`` returns for ``sliding_window_length=windows[k]``."""
        return self.native.operating_points(offsets, kind, windows, cutoffs, ignore_slices_after_accept, ignore_slices_after_accept)

    def operating_summary(self, offsets, kind, windows=OP_WINDOWS, cutoffs=CUTOFFS, ignore_slices_after_accept=25, stride=None, step_s=0.02,
                          target_faph=None):
        """The grid of ``operating_points`` summarised on the device (mww_stream_operating_summary; ``operating_summary_host`` is
        the host restatement): the dict of the operating-point grid without its per-track arrays - ``windows, cutoffs, counts,
        accepts, hours, usable, faph, frr, n_ambient, n_positive`` and, with ``target_faph``, ``target_faph, chosen,
        recommended, chosen_cutoff`` (``select_operating_points``).  What is read back does not grow with the tracks.
        ``stride`` defaults to the stream's own.  Raises ValueError without a positive (kind 1) track."""
        stride = self.stride if stride is None else int(stride)
        counts, accepts, hours, short, n_kind = self.native.operating_summary(
            offsets, kind, windows, cutoffs, ignore_slices_after_accept, ignore_slices_after_accept, stride, step_s)
        return _operating_summary(counts, accepts, hours, short, n_kind, windows, cutoffs, target_faph)

    def operating_bootstrap(self, offsets, kind, windows=OP_WINDOWS, cutoffs=CUTOFFS, ignore_slices_after_accept=25, stride=None, step_s=0.02,
                            target_faph=0.5, replicates=1000, seed=0, block=0, confidence=0.95, fixed=None, max_scratch_bytes=0):
        """``operating_summary`` with ``target_faph`` plus the bootstrap of its operating point on the device
        (mww_stream_operating_bootstrap; ``operating_bootstrap_host`` is the host restatement, the definitions stand above it):
        the summary's dict with ``bootstrap`` = dict(records, replicates, seed, block, confidence, fixed_row, fixed_cutoff,
        intervals).  ``records`` (native.BOOT_RECORD_DTYPE [replicates]) is all that is read back; ``intervals``
        (``bootstrap_intervals``) come from it on the host.  ``fixed``: a (row, cutoff index) of the grid, default the full
        data's recommended point (none when no window meets the target); ``block``: 0 or a multiple of
        native.BOOT_BLOCK_UNIT moving-average values."""
        stride = self.stride if stride is None else int(stride)
        if not 0 < float(confidence) < 1:
            raise ValueError("confidence must lie strictly between 0 and 1")
        summary = self.operating_summary(offsets, kind, windows, cutoffs, ignore_slices_after_accept, stride, step_s, target_faph)
        fixed = _bootstrap_fixed(summary, fixed)
        records = self.native.operating_bootstrap(offsets, kind, windows, cutoffs, ignore_slices_after_accept, ignore_slices_after_accept,
                                                  stride, step_s, target_faph, replicates, seed, block, fixed, max_scratch_bytes)
        return _bootstrap_result(summary, records, fixed, stride, step_s, replicates, seed, block, confidence)


def load_quantized(path):
    """the ``QuantizedModel`` (MixedNet), ``QuantizedMixedNetModel`` (MixedNet with residuals / a pooled head) or
    ``QuantizedGraphModel`` (Inception) of an ``.npz``; the files of the last two carry ``family``"""
    from . import quantize, quantize_graph, quantize_mixednet
    with np.load(path, allow_pickle=False) as z:
        family = str(z["family"]) if "family" in z.files else "mixednet"
    if family == quantize_mixednet.FAMILY:
        return quantize_mixednet.QuantizedMixedNetModel.load(path)
    return quantize_graph.QuantizedGraphModel.load(path) if family == quantize_graph.FAMILY else quantize.QuantizedModel.load(path)


class QuantizedStreamingModel(StreamingModel):
    """The int8 quantized streaming model (``--test_tflite_streaming_quantized``) with the methods of ``StreamingModel``:
    ``model_or_file`` is a ``quantize.QuantizedModel`` (MixedNet: the int8 kernel of csrc/tu_stream_q8.hip), a
    ``quantize_graph.QuantizedGraphModel`` (Inception: csrc/tu_stream_graph_q8.hip on a stream of
    ``mww_stream_create_convnet_q8``), a ``quantize_mixednet.QuantizedMixedNetModel`` (MixedNet with residuals / a pooled head:
    the <VAR> form of that kernel on a stream of ``mww_stream_create_mixednet_q8``) or the path of any one's ``.npz``; ``context`` is the float ``Model`` whose context
    (device, HIP stream, resident feature stores) the stream borrows.  Probabilities are ``uint8 / 255`` in float32
    (``read_q8`` gives the uint8 outputs), in the same device buffer the metrics kernel reads."""

    def __init__(self, model_or_file, stride: int, mode: str = "stream", context=None):
        from .quantize import QuantizedModel
        from .quantize_graph import QuantizedGraphModel
        from .quantize_mixednet import QuantizedMixedNetModel
        known = (QuantizedModel, QuantizedGraphModel, QuantizedMixedNetModel)
        q = model_or_file if isinstance(model_or_file, known) else load_quantized(model_or_file)
        if context is None:
            raise ValueError("QuantizedStreamingModel needs the float model whose context it shares (context=...)")
        if mode not in native.STREAM_MODES:
            raise ValueError("mode must be 'stream' or 'non_stream'")
        if int(stride) != int(q.desc["stride"]):
            raise ValueError("the streaming stride (%d) must be the quantized model's stride (%d)" % (stride, q.desc["stride"]))
        self.model = context
        self.quantized = q
        self.mode = mode
        self.stride = int(stride)
        self.frames = int(q.desc["frames"])
        self.desc = dict(q.desc, mode=mode)
        if isinstance(q, QuantizedGraphModel):
            self.native = native.GraphStream(context.engine, self.desc, int8=True)
        elif isinstance(q, QuantizedMixedNetModel):
            self.native = native.Stream(context.engine, self.desc, int8=True)
        else:
            self.native = native.Stream(context.engine, self.desc)
        self.native.set_quantized(*q.packed())

    def set_weights(self, weights):
        raise NotImplementedError("a quantized streaming model takes new parameters from quantize.quantize")

    def read_q8(self) -> np.ndarray:
        """uint8 outputs of the last call"""
        return self.native.read_q8()

    def get_state_q8(self) -> np.ndarray:
        """int8 rings (the layout of Stream.get_state)"""
        return self.native.get_state_q8()


# ------------------------------------------------------------------------------------------ restated post-processing

def moving_average(probabilities, sliding_window_length=5) -> np.ndarray:
    """``sliding_window_view(p, w).mean(axis=-1)`` on the float32 probabilities (test.py:349-352): float32 sums in order,
    divided by w.  Fewer than w probabilities give an empty array (the reference raises there; callers decide)."""
    p = np.asarray(probabilities, np.float32)
    if p.size < sliding_window_length:
        return np.zeros(0, np.float32)
    return np.lib.stride_tricks.sliding_window_view(p, sliding_window_length).mean(axis=-1)


def false_accept_counts(moving_averages: List[np.ndarray], cutoffs, ignore_slices_after_accept=25) -> np.ndarray:
    """The false-accept counts of test.py:119-135 at each cutoff, summed over the tracks (cooldown restarted per track)."""
    cutoffs = np.asarray(cutoffs, np.float64)
    counts = np.zeros(cutoffs.shape[0], np.uint64)
    for track in moving_averages:
        cooldown = np.full(cutoffs.shape[0], ignore_slices_after_accept, np.int64)
        for value in np.asarray(track, np.float32):
            cooldown = np.maximum(cooldown - 1, 0)
            hit = (cooldown == 0) & (np.float64(value) > cutoffs)
            counts += hit.astype(np.uint64)
            cooldown[hit] = ignore_slices_after_accept
    return counts


def moving_average_in_order(probabilities, sliding_window_length=5) -> np.ndarray:
    """The moving average as the kernels compute it, spelled out: the float32 sum p[i] + p[i+1] + ... taken in that order,
    then one float32 division by the window length.  Fewer than w probabilities give an empty array."""
    p = np.asarray(probabilities, np.float32)
    w = int(sliding_window_length)
    m = p.size - w + 1
    if m <= 0:
        return np.zeros(0, np.float32)
    s = np.zeros(m, np.float32)
    for k in range(w):
        s = s + p[k:k + m]
    return s / np.float32(w)


def detection_positions(moving_averages: List[np.ndarray], cutoff, ignore_slices_after_accept=25) -> List[np.ndarray]:
    """The loop of test.py:119-135 at one cutoff, recording WHERE it counts: per track the int64 indices of the moving
    average at which a false accept is counted (cooldown restarted per track).  ``len`` of each equals that track's share of
    ``false_accept_counts`` at the cutoff."""
    cutoff = float(cutoff)
    out = []
    for track in moving_averages:
        cooldown = ignore_slices_after_accept
        hits = []
        for i, value in enumerate(np.asarray(track, np.float32)):
            cooldown = max(cooldown - 1, 0)
            if cooldown == 0 and float(value) > cutoff:
                hits.append(i)
                cooldown = ignore_slices_after_accept
        out.append(np.array(hits, np.int64))
    return out


def detection_clips(windows, events, frames, stride, mode, sliding_window_length, before=0, after=0, return_kept=False):
    """The feature rows behind each detection as slices of the resident stores.  ``windows``: the tracks that were run
    (``FeatureHandler.track_windows``), ``events``: what ``detections`` returned for them.  The last probability of the
    event's averaging window is output n = index + w - 1 of its track; it was computed from the track rows ending at
    e = (n + 1) * stride (``mode="stream"``) or e = frames + n * stride (``"non_stream"``).  The clip is the track rows
    [e - frames - before, e + after) - with before = after = 0 exactly the window that fired - clipped to the rows the store
    holds: a track's ``pad_rows`` leading zero frames exist in no store.  Returns ``mww_window`` descriptors
    (store, 0, rows, 0, src_elem), empty clips dropped; with ``return_kept`` also the positions in ``events`` of the clips
    kept."""
    if mode not in native.STREAM_MODES:
        raise ValueError("mode must be 'stream' or 'non_stream'")
    win = np.ascontiguousarray(windows, native.WINDOW_DTYPE).reshape(-1)
    trk = np.asarray(events["track"], np.int64)
    n = np.asarray(events["index"], np.int64) + int(sliding_window_length) - 1
    end = (n + 1) * int(stride) if mode == "stream" else int(frames) + n * int(stride)
    pad = win["pad_rows"][trk].astype(np.int64)
    lo = np.maximum(end - int(frames) - int(before) - pad, 0)
    hi = np.minimum(end + int(after) - pad, win["copy_rows"][trk].astype(np.int64))
    keep = np.nonzero(hi > lo)[0]
    clips = np.zeros(keep.size, native.WINDOW_DTYPE)
    clips["store"] = win["store"][trk[keep]]
    clips["copy_rows"] = hi[keep] - lo[keep]
    clips["src_elem"] = win["src_elem"][trk[keep]] + lo[keep] * FEATURE_BINS
    return (clips, keep) if return_kept else clips


def track_hours(ma_lengths, stride=1, step_s=0.02) -> float:
    """test.py:117: sum of len(moving_average) * stride * step_s / 3600, accumulated in track order."""
    h = 0
    for n in ma_lengths:
        h += int(n) * stride * step_s / 3600.0
    return h


def false_accepts_per_hour(moving_averages: List[np.ndarray], cutoffs, ignore_slices_after_accept=75, stride=1, step_s=0.02):
    """test.py:94-137 ``compute_false_accepts_per_hour``."""
    counts = false_accept_counts(moving_averages, cutoffs, ignore_slices_after_accept)
    return counts.astype(np.float64) / track_hours([len(t) for t in moving_averages], stride, step_s)


def false_rejection_rates(scores, cutoffs) -> List[float]:
    """test.py:378-383: 1 - #{score > c} / N at each cutoff."""
    out = []
    for cutoff in cutoffs:
        true_accepts = sum(i > cutoff for i in scores)
        out.append(1 - true_accepts / len(scores))
    return out


def roc_curve(false_accepts_per_hour, false_rejections, cutoffs, max_faph=2.0):
    """test.py:140-204 ``generate_roc_curve``, bug for bug."""
    if false_accepts_per_hour[0] > max_faph:
        index_of_first_viable = 1
        while false_accepts_per_hour[index_of_first_viable] > max_faph:
            index_of_first_viable += 1
        x0 = false_accepts_per_hour[index_of_first_viable - 1]
        y0 = false_rejections[index_of_first_viable - 1]
        x1 = false_accepts_per_hour[index_of_first_viable]
        y1 = false_rejections[index_of_first_viable - 1]   # (sic: index - 1)
        fnr_at_max_faph = (y0 * (x1 - 2.0) + y1 * (2.0 - x0)) / (x1 - x0)   # (sic: the literal 2.0)
        cutoff_at_max_faph = (cutoffs[index_of_first_viable] + cutoffs[index_of_first_viable - 1]) / 2.0
    else:
        index_of_first_viable = 0
        fnr_at_max_faph = false_rejections[index_of_first_viable]
        cutoff_at_max_faph = cutoffs[index_of_first_viable]
    xs, ys, cs = [max_faph], [fnr_at_max_faph], [cutoff_at_max_faph]
    for index in range(index_of_first_viable, len(false_rejections)):
        if false_accepts_per_hour[index] != xs[-1]:
            xs.append(false_accepts_per_hour[index])
            ys.append(false_rejections[index])
            cs.append(cutoffs[index])
    if xs[-1] > 0:
        xs.append(0.0)
        ys.append(1.0)
        cs.append(0.0)
    return np.flip(xs), np.flip(ys), np.flip(cs)


def roc_text(x, y, cutoffs_at_points):
    """The file of test.py:392-401 and its AUC (trapezoid(y, x))."""
    from .train import _trapezoid
    auc = _trapezoid(y, x)
    lines = ["AUC {:.5f}".format(auc)]
    for i in range(0, x.shape[0]):
        lines.append("Cutoff {:.2f}: frr={:.4f}; faph={:.3f}".format(cutoffs_at_points[i], y[i], x[i]))
    return auc, "".join(line + "\n" for line in lines)


def evaluate_probabilities(ambient_probabilities, positive_probabilities, stride=1, step_s=0.02, sliding_window_length=5,
                           ignore_slices_after_accept=25, cutoffs=CUTOFFS):
    """Host restatement of test.py:340-401 on given per-track probabilities: returns dict(counts, faph, frr, x, y, cutoffs,
    auc, text)."""
    amb = []
    for i, p in enumerate(ambient_probabilities):
        ma = moving_average(p, sliding_window_length)
        if ma.size == 0:
            raise ValueError("ambient track %d has %d probabilities, fewer than the sliding window of %d" % (i, len(p), sliding_window_length))
        amb.append(ma)
    counts = false_accept_counts(amb, cutoffs, ignore_slices_after_accept)
    faph = counts.astype(np.float64) / track_hours([a.size for a in amb], stride, step_s)
    scores = []
    for i, p in enumerate(positive_probabilities):
        ma = moving_average(np.asarray(p, np.float32)[ignore_slices_after_accept:], sliding_window_length)
        if ma.size == 0:
            raise ValueError("positive track %d has no moving-average value after skipping %d probabilities" % (i, ignore_slices_after_accept))
        scores.append(np.max(ma))
    return _finish(counts, faph, scores, cutoffs)


def _finish(counts, faph, scores, cutoffs):
    if not scores:
        raise ValueError("the test set has no positive track")
    frr = false_rejection_rates(scores, cutoffs)
    x, y, c = roc_curve(faph, frr, cutoffs)
    auc, text = roc_text(x, y, c)
    return dict(counts=counts, faph=faph, frr=np.asarray(frr, np.float64), scores=np.asarray(scores, np.float32), x=x, y=y,
                cutoffs=c, auc=auc, text=text)


def streaming_model_roc(config, folder, streaming_model: StreamingModel, data_processor, data_set="testing",
                        ambient_set="testing_ambient", accuracy_name="tflite_streaming_roc.txt", sliding_window_length=5,
                        ignore_slices_after_accept=25, detections_cutoff=None):
    """test.py:293-403 ``tflite_streaming_model_roc`` on the device: the ambient tracks, then the positive tracks of
    ``data_set``, through one stream whose state carries over (stream mode; starting from the state it has - a fresh
    ``StreamingModel`` starts from zeros, as the reference's interpreter does), the moving averages / cooldown counts /
    scores by the metrics kernel.  Writes ``<train_dir>/<folder>/<accuracy_name>`` and returns the AUC.
    ``detections_cutoff`` (``--detections_cutoff``): additionally locates, on the same probabilities, every ambient false
    accept and every positive whose score is not above that cutoff (``detections_report``) and writes ``detections.txt`` /
    ``detections.npz`` into the same folder; the ROC file does not change."""
    stride = int(config["stride"])
    step_s = config["window_step_ms"] / 1000
    sm = streaming_model
    off, _ = sm.predict_tracks(data_processor, ambient_set)
    n_amb = off.size - 1
    counts = np.zeros(CUTOFFS.size, np.uint64)
    hours = 0
    if n_amb:
        counts, ma_len, _ = sm.metrics(off, np.zeros(n_amb, np.int32), CUTOFFS, sliding_window_length, ignore_slices_after_accept)
        bad = np.nonzero(ma_len == 0)[0]
        if bad.size:
            raise ValueError("ambient track %d of %r has fewer than %d probabilities" % (bad[0], ambient_set, sliding_window_length))
        hours = track_hours(ma_len, stride, step_s)
    located = {}
    if detections_cutoff is not None and n_amb:
        located["ambient"] = sm.detections(off, np.zeros(n_amb, np.int32), detections_cutoff, sliding_window_length, ignore_slices_after_accept)
    faph = counts.astype(np.float64) / hours
    off, _ = sm.predict_tracks(data_processor, data_set, only_label=1.0)
    n_pos = off.size - 1
    scores = []
    if n_pos:
        _, ma_len, score = sm.metrics(off, np.ones(n_pos, np.int32), CUTOFFS, sliding_window_length, ignore_slices_after_accept)
        bad = np.nonzero(ma_len == 0)[0]
        if bad.size:
            raise ValueError("positive track %d of %r has no moving-average value after skipping %d probabilities"
                             % (bad[0], data_set, ignore_slices_after_accept))
        scores = list(score)
        if detections_cutoff is not None:
            located["positive"] = sm.detections(off, np.ones(n_pos, np.int32), detections_cutoff, sliding_window_length, ignore_slices_after_accept)
    res = _finish(counts, faph, scores, CUTOFFS)
    path = os.path.join(config["train_dir"], folder)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, accuracy_name), "wt") as fd:
        fd.write(res["text"])
    if detections_cutoff is not None:
        text, arrays = detections_report(located.get("ambient"), located.get("positive"), detections_cutoff, stride, step_s)
        with open(os.path.join(path, "detections.txt"), "wt") as fd:
            fd.write(text)
        np.savez(os.path.join(path, "detections.npz"), **arrays)
    return res["auc"]


# ------------------------------------------------------------------------------------------ choosing what to ship

def select_operating_points(faph, frr, usable, target_faph, windows=None):
    """The selection rule of the operating-point grid, on ``faph [W, C]`` / ``frr [W, C]`` (cutoffs ascending along C),
    ``usable [W]`` and the rows' window sizes (default: ascending with the row).  Per usable window the chosen cutoff is the
    smallest one with ``faph <= target_faph`` there AND at every larger cutoff of the grid (under a cooldown the counts need
    not fall monotonically with the cutoff, so the first crossing is not enough); -1 when even the largest cutoff exceeds
    the target, and for an unusable window.  The recommendation is the window whose chosen cutoff has the smallest FRR; ties
    go to the smaller FAPH, then to the smaller window (then the earlier row).  Returns ``(chosen [W] int64, recommended)``,
    ``recommended`` a row or -1 when no window meets the target; raises ValueError when no window is usable."""
    faph, frr, usable = np.asarray(faph, np.float64), np.asarray(frr, np.float64), np.asarray(usable, bool)
    if not usable.any():
        raise ValueError("no window of the grid is usable: every one is longer than an ambient track or leaves a positive track without a value")
    chosen = np.full(faph.shape[0], -1, np.int64)
    for k in np.nonzero(usable)[0]:
        above = np.nonzero(~(faph[k] <= target_faph))[0]
        first = above[-1] + 1 if above.size else 0
        if first < faph.shape[1]:
            chosen[k] = first
    windows = np.arange(chosen.size) if windows is None else np.asarray(windows, np.int64)
    best = [(frr[k, chosen[k]], faph[k, chosen[k]], int(windows[k]), k) for k in range(chosen.size) if chosen[k] >= 0]
    return chosen, (min(best)[3] if best else -1)


def _rates_and_selection(windows, cutoffs, counts, hours, usable, frr_row, target_faph, n_pos, after_counts=(), last=()):
    """Where the grid and the summary end, on ``windows`` int64 [W] and ``cutoffs`` float64 [C]: FAPH and FRR of the usable
    windows (``frr_row(k)``: the FRR of window k at every cutoff), the dict - the caller's own entries ``after_counts`` behind
    ``counts`` and ``last`` at the end, the order the two dicts always had - and with ``target_faph`` the selection."""
    if n_pos == 0:
        raise ValueError("the test set has no positive track")
    usable = np.asarray(usable, bool)
    faph = np.full((windows.size, cutoffs.size), np.nan)
    frr = np.full((windows.size, cutoffs.size), np.nan)
    for k in np.nonzero(usable)[0]:
        faph[k] = counts[k].astype(np.float64) / hours[k]
        frr[k] = frr_row(k)
    out = dict(windows=windows, cutoffs=cutoffs, counts=np.asarray(counts, np.uint64), **dict(after_counts))
    out.update(hours=np.asarray(hours, np.float64), usable=usable, faph=faph, frr=frr, **dict(last))
    if target_faph is not None:
        chosen, rec = select_operating_points(faph, frr, usable, target_faph, windows)
        out.update(target_faph=float(target_faph), chosen=chosen, recommended=int(rec),
                   chosen_cutoff=np.array([cutoffs[c] if c >= 0 else np.nan for c in chosen], np.float64))
    return out


def _operating_grid(counts, ambient_ma_len, positive_ma_len, score, windows, cutoffs, stride, step_s, target_faph):
    """counts [W, C], ambient_ma_len [W, n_amb], positive_ma_len / score [W, n_pos] -> the grid's dict (both paths end here)"""
    windows, cutoffs = np.asarray(windows, np.int64).reshape(-1), np.asarray(cutoffs, np.float64).reshape(-1)
    W = windows.size
    hours = np.array([track_hours(ambient_ma_len[k], stride, step_s) for k in range(W)], np.float64)
    usable = [ambient_ma_len.shape[1] > 0 and bool(np.all(ambient_ma_len[k] > 0)) and bool(np.all(positive_ma_len[k] > 0)) for k in range(W)]
    return _rates_and_selection(windows, cutoffs, counts, hours, usable, lambda k: false_rejection_rates(list(score[k]), cutoffs),
                                target_faph, score.shape[1],
                                last=dict(ambient_ma_len=np.asarray(ambient_ma_len, np.int64),
                                          positive_ma_len=np.asarray(positive_ma_len, np.int64), score=np.asarray(score, np.float32)))


def operating_points_host(ambient_probabilities, positive_probabilities, windows=OP_WINDOWS, cutoffs=CUTOFFS, stride=1, step_s=0.02,
                          ignore_slices_after_accept=25, target_faph=None, skip=None):
    """Host restatement of the operating-point grid on given per-track probabilities, from ``moving_average_in_order``,
    ``false_accept_counts`` and ``false_rejection_rates``: per window of ``windows`` the ambient tracks' cooldown counts at
    each cutoff, the positive tracks' scores after the first ``skip`` (default: ``ignore_slices_after_accept``)
    probabilities, FAPH and FRR; with ``target_faph`` also the selection (``select_operating_points``).  Returns the dict
    ``operating_point_grid`` returns."""
    skip = ignore_slices_after_accept if skip is None else skip
    windows = [int(w) for w in windows]
    n_amb, n_pos = len(ambient_probabilities), len(positive_probabilities)
    counts = np.zeros((len(windows), len(cutoffs)), np.uint64)
    amb_len, pos_len = np.zeros((len(windows), n_amb), np.int64), np.zeros((len(windows), n_pos), np.int64)
    score = np.zeros((len(windows), n_pos), np.float32)
    done = {}
    for k, w in enumerate(windows):
        if w not in done:   # a window may repeat
            amb = [moving_average_in_order(p, w) for p in ambient_probabilities]
            pos = [moving_average_in_order(np.asarray(p, np.float32)[skip:], w) for p in positive_probabilities]
            done[w] = (false_accept_counts(amb, cutoffs, ignore_slices_after_accept), [a.size for a in amb], [a.size for a in pos],
                       [np.max(a) if a.size else np.float32(-np.inf) for a in pos])
        counts[k], amb_len[k], pos_len[k], score[k] = done[w]
    return _operating_grid(counts, amb_len, pos_len, score, windows, cutoffs, stride, step_s, target_faph)


SUMMARY_KEYS = ("windows", "cutoffs", "counts", "accepts", "hours", "usable", "faph", "frr", "n_ambient", "n_positive")
SELECTION_KEYS = ("target_faph", "chosen", "recommended", "chosen_cutoff")


def _operating_summary(counts, accepts, hours, short_tracks, n_kind, windows, cutoffs, target_faph):
    """what mww_stream_operating_summary returns -> the summary's dict: the rules of ``_operating_grid`` on the reduced numbers"""
    windows, cutoffs = np.asarray(windows, np.int64).reshape(-1), np.asarray(cutoffs, np.float64).reshape(-1)
    n_amb, n_pos = int(n_kind[0]), int(n_kind[1])
    usable = [n_amb > 0 and short_tracks[k, 0] == 0 and short_tracks[k, 1] == 0 for k in range(windows.size)]
    # false_rejection_rates: 1 - true_accepts / len(scores)
    return _rates_and_selection(windows, cutoffs, counts, hours, usable, lambda k: 1 - accepts[k].astype(np.float64) / n_pos,
                                target_faph, n_pos, after_counts=dict(accepts=np.asarray(accepts, np.uint64)),
                                last=dict(n_ambient=n_amb, n_positive=n_pos))


def operating_summary_host(ambient_probabilities, positive_probabilities, windows=OP_WINDOWS, cutoffs=CUTOFFS, stride=1, step_s=0.02,
                           ignore_slices_after_accept=25, target_faph=None, skip=None):
    """Host restatement of ``StreamingModel.operating_summary`` on given per-track probabilities: ``operating_points_host``
    with the per-track arrays reduced - ``accepts[k, c]`` counts the scores of window k with ``float64(score) > cutoffs[c]`` -
    and its counts, hours, usable, faph and frr (so ``false_rejection_rates`` and ``track_hours``) taken as they are."""
    g = operating_points_host(ambient_probabilities, positive_probabilities, windows, cutoffs, stride, step_s, ignore_slices_after_accept,
                              target_faph, skip)
    score = g["score"].astype(np.float64)
    accepts = np.array([[np.count_nonzero(score[k] > c) for c in g["cutoffs"]] for k in range(score.shape[0])], np.uint64)
    out = {k: g[k] for k in ("windows", "cutoffs", "counts", "hours", "usable", "faph", "frr")}
    out.update(accepts=accepts.reshape(g["counts"].shape), n_ambient=len(ambient_probabilities), n_positive=len(positive_probabilities))
    out.update({k: g[k] for k in SELECTION_KEYS if k in g})
    return out


# ---- bootstrap of the operating point (mww_stream_operating_bootstrap).  The definitions, once:
#   units    a positive unit is a positive track.  An ambient unit is a block of an ambient track: with block = 0 every track
#            is one block, an empty one too; with block = L > 0 (a multiple of native.BOOT_BLOCK_UNIT) a track of n
#            probabilities has ceil(n / L) blocks, whatever the window, and at window k block b owns the moving-average indices
#            [b L, min((b + 1) L, m_k)), possibly none.  A block's count at (k, c) is the number of the track's detections -
#            those of the whole-track cooldown walk, so the cooldown carries across block borders and the blocks of a track
#            sum to its count - whose index it owns; its length at k is the size of its index range.  NB blocks in all, in
#            (track, block) order.
#   draws    ``bootstrap_draw``; replicate r draws the NB blocks draw(seed, 0, r, i, NB) and the n_pos positives
#            draw(seed, 1, r, i, n_pos); one set of draws serves all windows.
#   grid     counts_r[k, c]: the sum of the drawn blocks' counts; slices_r[k]: the sum of their lengths; accepts_r[k, c]: the
#            drawn positives with float64(score[k, t]) > cutoffs[c]; hours_r = ((slices_r * stride) * step_s) / 3600.0,
#            faph_r = float64(counts_r) / hours_r, frr_r = 1 - float64(accepts_r) / n_pos; a window is usable in a replicate
#            when it is usable on the full data and slices_r[k] > 0.
#   records  per replicate the point ``select_operating_points(faph_r, frr_r, usable_r, target_faph, windows)`` re-selects
#            ((-1, -1) when no window meets the target) with counts_r, slices_r, accepts_r there, and the same three at a fixed
#            point of the grid.  The re-selected point gives the uncertainty of the metric a selection rests on, the fixed
#            point that of the cutoff that ships.
#   intervals  ``bootstrap_intervals``: percentiles of the sorted replicate values.
# What the intervals are not: blocks of one recording are not independent (a block bootstrap only keeps the dependence inside
# a block); with few ambient tracks and block = 0 the FAPH interval is coarse (it takes few distinct values); percentile
# intervals are not bias-corrected.

def bootstrap_draw(seed, kind, r, i, n):
    """Draw ``i`` (an integer or an array of them, < 2^32) of replicate ``r`` (< 2^16 here, < 2^24 by the layout) for
    ``kind`` (0: ambient blocks, 1: positives) out of ``n`` (< 2^32) units, int64 in 0 .. n - 1: the counter
    ``kind << 56 | r << 32 | i`` times 0x9E3779B97F4A7C15 plus ``seed`` (mod 2^64) through the splitmix64 finaliser, then
    ``((z >> 32) * n) >> 32``.  A multiply-shift without rejection: the bias is below n / 2^32."""
    u = np.uint64
    idx = np.atleast_1d(np.asarray(i)).astype(np.uint64)
    ctr = np.full(idx.shape, (int(kind) << 56) | (int(r) << 32), np.uint64) | idx
    z = np.full(idx.shape, int(seed) & (2 ** 64 - 1), np.uint64) + ctr * u(0x9E3779B97F4A7C15)   # arrays wrap mod 2^64
    z ^= z >> u(30)
    z *= u(0xBF58476D1CE4E5B9)
    z ^= z >> u(27)
    z *= u(0x94D049BB133111EB)
    z ^= z >> u(31)
    out = (((z >> u(32)) * u(int(n))) >> u(32)).astype(np.int64)
    return out.reshape(np.shape(i)) if np.ndim(i) else int(out[0])


def bootstrap_block_counts(moving_average_values, cutoffs, ignore_slices_after_accept, block, n_blocks):
    """One ambient track's detections per block, uint32 [n_blocks, C]: ``detection_positions`` at every cutoff at once (the loop
    of test.py:119-135 on a vector of cooldowns, as ``false_accept_counts`` runs it), each detection counted in block
    ``index // block`` (``block`` 0: the one block)."""
    cutoffs = np.asarray(cutoffs, np.float64)
    out = np.zeros((n_blocks, cutoffs.shape[0]), np.uint32)
    cooldown = np.full(cutoffs.shape[0], ignore_slices_after_accept, np.int64)
    for i, value in enumerate(np.asarray(moving_average_values, np.float32)):
        cooldown = np.maximum(cooldown - 1, 0)
        hit = (cooldown == 0) & (np.float64(value) > cutoffs)
        out[i // block if block else 0] += hit.astype(np.uint32)
        cooldown[hit] = ignore_slices_after_accept
    return out


def bootstrap_units_host(ambient_probabilities, positive_probabilities, windows, cutoffs, ignore_slices_after_accept=25, block=0, skip=None):
    """The units of the bootstrap on given per-track probabilities: ``(blk_cnt uint32 [W, NB, C], blk_len int64 [W, NB],
    score float32 [W, n_pos])`` from ``moving_average_in_order`` and the detections binned by ``index // block``."""
    block = int(block)
    if block < 0 or block % native.BOOT_BLOCK_UNIT:
        raise ValueError("block must be 0 or a positive multiple of %d" % native.BOOT_BLOCK_UNIT)
    skip = ignore_slices_after_accept if skip is None else skip
    windows = [int(w) for w in windows]
    n_blocks = [(-(-len(p) // block) if block else 1) for p in ambient_probabilities]
    first = np.concatenate([[0], np.cumsum(n_blocks)]).astype(np.int64)
    blk_cnt = np.zeros((len(windows), int(first[-1]), len(cutoffs)), np.uint32)
    blk_len = np.zeros((len(windows), int(first[-1])), np.int64)
    score = np.zeros((len(windows), len(positive_probabilities)), np.float32)
    done = {}
    for k, w in enumerate(windows):
        if w in done:   # a window may repeat
            blk_cnt[k], blk_len[k], score[k] = blk_cnt[done[w]], blk_len[done[w]], score[done[w]]
            continue
        done[w] = k
        for j, p in enumerate(ambient_probabilities):
            ma = moving_average_in_order(p, w)
            blk_cnt[k, first[j]:first[j + 1]] = bootstrap_block_counts(ma, cutoffs, ignore_slices_after_accept, block, n_blocks[j])
            for b in range(n_blocks[j]):
                blk_len[k, first[j] + b] = max(min((b + 1) * block, ma.size) - b * block, 0) if block else ma.size
        pos = [moving_average_in_order(np.asarray(p, np.float32)[skip:], w) for p in positive_probabilities]
        score[k] = [np.max(a) if a.size else np.float32(-np.inf) for a in pos]
    return blk_cnt, blk_len, score


def bootstrap_records_host(units, usable, windows, cutoffs, stride, step_s, target_faph, replicates, seed, fixed=None,
                           select=select_operating_points):
    """The records of ``replicates`` replicates on the units of ``bootstrap_units_host`` (``usable``: the windows usable on the
    full data): native.BOOT_RECORD_DTYPE [replicates], what mww_stream_operating_bootstrap writes.  ``select``: the selection
    rule (a test compares another)."""
    blk_cnt, blk_len, score = units
    cutoffs = np.asarray(cutoffs, np.float64).reshape(-1)
    if np.any(~(np.diff(cutoffs) > 0)):
        raise ValueError("the cutoffs of a bootstrap must ascend strictly")
    if not 1 <= int(replicates) <= native.BOOT_MAX_REPLICATES:
        raise ValueError("replicates must lie in 1..%d" % native.BOOT_MAX_REPLICATES)
    W, NB, C = blk_cnt.shape
    n_pos = score.shape[1]
    score64 = score.astype(np.float64)
    rec = np.zeros(int(replicates), native.BOOT_RECORD_DTYPE)
    for r in range(int(replicates)):
        d = bootstrap_draw(seed, 0, r, np.arange(NB), NB)
        counts = blk_cnt[:, d, :].astype(np.uint64).sum(axis=1, dtype=np.uint64)
        slices = blk_len[:, d].sum(axis=1, dtype=np.int64)
        t = bootstrap_draw(seed, 1, r, np.arange(n_pos), n_pos)
        accepts = np.array([np.count_nonzero(score64[k, t][:, None] > cutoffs[None, :], axis=0) for k in range(W)], np.uint64).reshape(W, C)
        usable_r = np.asarray(usable, bool) & (slices > 0)
        faph, frr = np.full((W, C), np.nan), np.full((W, C), np.nan)
        for k in np.nonzero(usable_r)[0]:
            faph[k] = counts[k].astype(np.float64) / (int(slices[k]) * stride * step_s / 3600.0)
            frr[k] = 1 - accepts[k].astype(np.float64) / n_pos
        row = col = -1
        if usable_r.any():
            chosen, row = select(faph, frr, usable_r, target_faph, windows)
            col = int(chosen[row]) if row >= 0 else -1
        rec[r]["sel_row"], rec[r]["sel_cutoff"] = row, col
        if row >= 0:
            rec[r]["sel_counts"], rec[r]["sel_slices"], rec[r]["sel_accepts"] = counts[row, col], slices[row], accepts[row, col]
        if fixed is not None:
            rec[r]["fixed_counts"], rec[r]["fixed_slices"], rec[r]["fixed_accepts"] = counts[tuple(fixed)], slices[fixed[0]], accepts[tuple(fixed)]
    return rec


def bootstrap_intervals(records, n_positive, stride, step_s, confidence=0.95, fixed=True):
    """Percentile intervals from the records: for confidence q and the sorted replicate values v[0 .. R - 1],
    ``lower = v[floor((1 - q) / 2 * R)]``, ``upper = v[ceil((1 + q) / 2 * R) - 1]``.  At the fixed point: ``recall`` (1 - frr)
    and ``false_accepts_per_hour`` (+inf in a replicate that drew no ambient time); re-selected per replicate:
    ``recall_at_target`` and ``false_accepts_per_hour_at_target``, a replicate without a point counting as recall 0 and FAPH
    +inf.  -> dict name -> (lower, upper); the fixed-point entries are None without a fixed point.  These are plain percentile
    intervals, not bias-corrected."""
    q = float(confidence)
    if not 0 < q < 1:
        raise ValueError("confidence must lie strictly between 0 and 1")
    R = records.shape[0]
    # the two products up to 1e-9: in float64 (1 - 0.9) / 2 * 40 falls just short of 2
    lo = min(max(int(np.floor((1 - q) / 2 * R + 1e-9)), 0), R - 1)
    hi = min(max(int(np.ceil((1 + q) / 2 * R - 1e-9)) - 1, 0), R - 1)

    def series(prefix, has_point):
        hours = records[prefix + "_slices"].astype(np.int64) * stride * step_s / 3600.0
        with np.errstate(divide="ignore", invalid="ignore"):
            faph = np.where(has_point & (hours > 0), records[prefix + "_counts"].astype(np.float64) / hours, np.inf)
        recall = np.where(has_point, 1 - (1 - records[prefix + "_accepts"].astype(np.float64) / n_positive), 0.0)
        return [(float(np.sort(v)[lo]), float(np.sort(v)[hi])) for v in (recall, faph)]

    at_target = series("sel", records["sel_row"] >= 0)
    at_fixed = series("fixed", np.ones(R, bool)) if fixed else [None, None]
    return dict(recall=at_fixed[0], false_accepts_per_hour=at_fixed[1], recall_at_target=at_target[0],
                false_accepts_per_hour_at_target=at_target[1])


def _bootstrap_fixed(summary, fixed):
    """the fixed point of a bootstrap: the given (row, cutoff index), else the full data's recommended point, else None"""
    if fixed is not None:
        return int(fixed[0]), int(fixed[1])
    r = summary["recommended"]
    return (int(r), int(summary["chosen"][r])) if r >= 0 else None


def _bootstrap_result(summary, records, fixed, stride, step_s, replicates, seed, block, confidence):
    out = dict(summary)
    out["bootstrap"] = dict(records=records, replicates=int(replicates), seed=int(seed), block=int(block), confidence=float(confidence),
                            fixed_row=fixed[0] if fixed else -1, fixed_cutoff=fixed[1] if fixed else -1,
                            intervals=bootstrap_intervals(records, summary["n_positive"], stride, step_s, confidence, fixed is not None))
    return out


def operating_bootstrap_host(ambient_probabilities, positive_probabilities, windows=OP_WINDOWS, cutoffs=CUTOFFS, stride=1, step_s=0.02,
                             ignore_slices_after_accept=25, target_faph=0.5, replicates=1000, seed=0, block=0, confidence=0.95,
                             fixed=None, skip=None, units=None):
    """Host restatement of ``StreamingModel.operating_bootstrap`` on given per-track probabilities, by the definitions above:
    ``operating_summary_host`` plus ``bootstrap`` (records, settings, intervals).  ``units``: those of ``bootstrap_units_host``
    on the same inputs, when the caller has them already."""
    summary = operating_summary_host(ambient_probabilities, positive_probabilities, windows, cutoffs, stride, step_s,
                                     ignore_slices_after_accept, target_faph, skip)
    if units is None:
        units = bootstrap_units_host(ambient_probabilities, positive_probabilities, windows, cutoffs, ignore_slices_after_accept, block, skip)
    fixed = _bootstrap_fixed(summary, fixed)
    records = bootstrap_records_host(units, summary["usable"], summary["windows"], cutoffs, stride, step_s, target_faph, replicates, seed, fixed)
    return _bootstrap_result(summary, records, fixed, stride, step_s, replicates, seed, block, confidence)


def operating_point_text(grid):
    """``operating_points.txt``: one line per window, then the recommendation"""
    lines = []
    for k, w in enumerate(grid["windows"]):
        c = grid["chosen"][k]
        if not grid["usable"][k]:
            lines.append("Window {}: unusable (longer than an ambient track, or no value left on a positive track)".format(w))
        elif c < 0:
            lines.append("Window {}: no cutoff of the grid keeps faph <= {:g}".format(w, grid["target_faph"]))
        else:
            lines.append("Window {}: cutoff={:.2f}; faph={:.3f}; frr={:.4f}".format(w, grid["cutoffs"][c], grid["faph"][k, c], grid["frr"][k, c]))
    r = grid["recommended"]
    if r < 0:
        lines.append("Recommended: none (no window keeps faph <= {:g})".format(grid["target_faph"]))
    else:
        c = grid["chosen"][r]
        lines.append("Recommended: window {}, cutoff {:.2f} (faph={:.3f}; frr={:.4f}) for faph <= {:g}".format(
            grid["windows"][r], grid["cutoffs"][c], grid["faph"][r, c], grid["frr"][r, c], grid["target_faph"]))
    return "".join(line + "\n" for line in lines)


def operating_point_settings(grid, mode, quantized):
    """``operating_point.json``: the recommendation as plain settings (None where no window meets the target)"""
    r = grid["recommended"]
    c = grid["chosen"][r] if r >= 0 else -1
    return {"probability_cutoff": float(grid["cutoffs"][c]) if r >= 0 else None,
            "sliding_window_size": int(grid["windows"][r]) if r >= 0 else None,
            "false_accepts_per_hour": float(grid["faph"][r, c]) if r >= 0 else None,
            "false_rejection_rate": float(grid["frr"][r, c]) if r >= 0 else None,
            "target_false_accepts_per_hour": float(grid["target_faph"]), "mode": mode, "quantized": bool(quantized)}


def operating_point_grid(config, folder, sm, data_processor, target_faph, windows=OP_WINDOWS, data_set="testing",
                         ambient_set="testing_ambient", ignore_slices_after_accept=25):
    """FAPH / FRR at every (sliding window, cutoff) of ``windows`` x ``CUTOFFS`` and the operating point for
    ``target_faph``: the tracks are fed as ``streaming_model_roc`` feeds them (the ambient tracks, then the positive tracks
    of ``data_set``, the ring state carried over, from the state the stream has), with one grid call per kind
    (``StreamingModel.operating_points``).  Writes ``operating_points.txt`` / ``operating_points.npz`` /
    ``operating_point.json`` into ``<train_dir>/<folder>`` and returns the grid (``operating_points_host`` is its host
    restatement); a window no track set supports is reported unusable and left out of the choice."""
    import json
    stride = int(config["stride"])
    step_s = config["window_step_ms"] / 1000
    windows = [int(w) for w in windows]
    off, _ = sm.predict_tracks(data_processor, ambient_set)
    n_amb = off.size - 1
    counts, amb_len = np.zeros((len(windows), CUTOFFS.size), np.uint64), np.zeros((len(windows), 0), np.int64)
    if n_amb:
        counts, amb_len, _ = sm.operating_points(off, np.zeros(n_amb, np.int32), windows, CUTOFFS, ignore_slices_after_accept)
    off, _ = sm.predict_tracks(data_processor, data_set, only_label=1.0)
    n_pos = off.size - 1
    pos_len, score = np.zeros((len(windows), 0), np.int64), np.zeros((len(windows), 0), np.float32)
    if n_pos:
        _, pos_len, score = sm.operating_points(off, np.ones(n_pos, np.int32), windows, CUTOFFS, ignore_slices_after_accept)
    grid = _operating_grid(counts, amb_len, pos_len, score, windows, CUTOFFS, stride, step_s, target_faph)
    path = os.path.join(config["train_dir"], folder)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "operating_points.txt"), "wt") as fd:
        fd.write(operating_point_text(grid))
    np.savez(os.path.join(path, "operating_points.npz"), **{k: grid[k] for k in
             ("windows", "cutoffs", "counts", "faph", "frr", "hours", "chosen_cutoff")}, recommended=np.int64(grid["recommended"]))
    with open(os.path.join(path, "operating_point.json"), "wt") as fd:
        json.dump(operating_point_settings(grid, sm.mode, isinstance(sm, QuantizedStreamingModel)), fd, indent=2)
        fd.write("\n")
    return grid


def operating_point_bootstrap(config, folder, sm, data_processor, target_faph, windows=OP_WINDOWS, bootstrap=None, data_set="testing",
                              ambient_set="testing_ambient", ignore_slices_after_accept=25):
    """The bootstrap of the operating point of ``operating_point_grid`` (``--operating_point_bootstrap``): the ambient tracks,
    then the positive tracks of ``data_set``, through ONE native run from the state the stream has - the order and the carried
    state of the grid's two runs, so the same probabilities -, then ``StreamingModel.operating_bootstrap`` with the settings
    ``bootstrap`` (``bootstrap_settings``; default ``BOOTSTRAP_DEFAULTS``).  Writes ``operating_point_bootstrap.json`` (settings,
    the fixed point, the intervals) and ``operating_point_bootstrap.npz`` (the records, field by field) into
    ``<train_dir>/<folder>`` and returns the dict of ``operating_bootstrap``; the grid's files are not touched."""
    import json
    b = dict(BOOTSTRAP_DEFAULTS, **(bootstrap or {}))
    windows = [int(w) for w in windows]
    amb, _ = data_processor.track_windows(ambient_set, sm.frames)
    pos, _ = data_processor.track_windows(data_set, sm.frames, only_label=1.0)
    offsets = sm.native.run(np.concatenate([amb, pos]))
    kind = np.concatenate([np.zeros(amb.size, np.int32), np.ones(pos.size, np.int32)])
    out = sm.operating_bootstrap(offsets, kind, windows, CUTOFFS, ignore_slices_after_accept, int(config["stride"]), config["window_step_ms"] / 1000,
                                 target_faph, b["replicates"], b["seed"], b["block"], b["confidence"])
    boot = out[BOOTSTRAP_KEY]
    r, c = boot["fixed_row"], boot["fixed_cutoff"]
    path = os.path.join(config["train_dir"], folder)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "operating_point_bootstrap.json"), "wt") as fd:
        json.dump({"replicates": boot["replicates"], "seed": boot["seed"], "block": boot["block"], "confidence": boot["confidence"],
                   "target_false_accepts_per_hour": float(target_faph),
                   "probability_cutoff": float(out["cutoffs"][c]) if r >= 0 else None,
                   "sliding_window_size": int(out["windows"][r]) if r >= 0 else None,
                   "intervals": {k: (list(v) if v is not None else None) for k, v in boot["intervals"].items()},
                   "replicates_without_operating_point": int(np.count_nonzero(boot["records"]["sel_row"] < 0)),
                   "mode": sm.mode, "quantized": isinstance(sm, QuantizedStreamingModel)}, fd, indent=2)
        fd.write("\n")
    np.savez(os.path.join(path, "operating_point_bootstrap.npz"), windows=out["windows"], cutoffs=out["cutoffs"],
             fixed=np.array([r, c], np.int64), **{name: boot["records"][name].copy() for name in native.BOOT_RECORD_DTYPE.names})
    return out


# ---- the training-loop option (train.train)
VALIDATION_KEY = "streaming_validation"
VALIDATION_DEFAULTS = dict(windows=[5], mode="stream", ignore_slices_after_accept=25, data_set="validation", ambient_set="validation_ambient",
                           every_evals=1)
STREAMING_METRICS = ("streaming_recall", "streaming_false_rejection_rate", "streaming_false_accepts_per_hour", "streaming_cutoff",
                     "streaming_window", "streaming_hours", "streaming_positives")
# ... and, with a ``bootstrap`` sub-mapping, the percentile bounds of ``bootstrap_intervals``: recall and FAPH at the full data's
# operating point (the cutoff that would ship), recall at the point each replicate re-selects (the metric the loop selects on)
BOOTSTRAP_KEY = "bootstrap"
BOOTSTRAP_DEFAULTS = dict(replicates=1000, seed=0, confidence=0.95, block=0)
STREAMING_BOOTSTRAP_METRICS = ("streaming_recall_lower", "streaming_recall_upper", "streaming_false_accepts_per_hour_lower",
                               "streaming_false_accepts_per_hour_upper", "streaming_recall_at_target_lower",
                               "streaming_recall_at_target_upper")
STREAMING_METRIC_NAMES = STREAMING_METRICS + STREAMING_BOOTSTRAP_METRICS   # what the best-weights rule may name


def bootstrap_settings(key, given):
    """The ``bootstrap`` sub-mapping of ``streaming_validation`` (``replicates``, ``seed``, ``confidence``, ``block``) with its
    defaults filled in; a ValueError names ``key``, the sub-mapping and the bad key."""
    name = "%s: %s" % (key, BOOTSTRAP_KEY)
    if not isinstance(given, dict):
        raise ValueError("%s must be a mapping (%s)" % (name, ", ".join(BOOTSTRAP_DEFAULTS)))
    unknown = sorted(set(given) - set(BOOTSTRAP_DEFAULTS), key=str)
    if unknown:
        raise ValueError("%s: unknown key(s) %s; known: %s" % (name, ", ".join(map(str, unknown)), ", ".join(BOOTSTRAP_DEFAULTS)))
    b = dict(BOOTSTRAP_DEFAULTS, **given)
    integer = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))   # noqa: E731
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))   # noqa: E731
    bad = [k for k, ok in (("replicates", integer(b["replicates"]) and 1 <= b["replicates"] <= native.BOOT_MAX_REPLICATES),
                           ("seed", integer(b["seed"]) and 0 <= b["seed"] < 2 ** 64),
                           ("confidence", number(b["confidence"]) and 0 < b["confidence"] < 1),
                           ("block", integer(b["block"]) and b["block"] >= 0 and b["block"] % native.BOOT_BLOCK_UNIT == 0)) if not ok]
    if bad:
        raise ValueError("%s: %s out of range (replicates an integer in 1..%d; seed an integer in 0 .. 2^64 - 1; confidence strictly "
                         "between 0 and 1; block 0 or a positive multiple of %d moving-average values)"
                         % (name, ", ".join(bad), native.BOOT_MAX_REPLICATES, native.BOOT_BLOCK_UNIT))
    return dict(replicates=int(b["replicates"]), seed=int(b["seed"]), confidence=float(b["confidence"]), block=int(b["block"]))


def streaming_validation_config(config, world=1):
    """The ``streaming_validation`` mapping of a training configuration with its defaults filled in, or None without the key.
    Unknown keys, out-of-range values and a world size above 1 are ``ValueError``s that name the key; so is a
    ``minimization_metric`` / ``maximization_metric`` that names a streaming metric without the key, or one of
    ``STREAMING_BOOTSTRAP_METRICS`` without the ``bootstrap`` sub-mapping.  The normalised mapping has a ``bootstrap`` entry
    (``bootstrap_settings``) only when the configuration gives one."""
    key = VALIDATION_KEY
    given = config.get(key)
    if given is None:
        named = [config.get(k) for k in ("minimization_metric", "maximization_metric") if config.get(k) in STREAMING_METRIC_NAMES]
        if named:
            raise ValueError("%s: the metric %s needs the %s mapping (target_faph, ...)" % (key, ", ".join(named), key))
        return None
    if not isinstance(given, dict):
        raise ValueError("%s must be a mapping (target_faph, windows, ...)" % key)
    from .quantize import LOOP_DEFAULTS, loop_settings
    unknown = sorted(set(given) - set(VALIDATION_DEFAULTS) - set(LOOP_DEFAULTS) - {"target_faph", BOOTSTRAP_KEY}, key=str)
    if unknown:
        raise ValueError("%s: unknown key(s) %s; known: target_faph, %s" % (key, ", ".join(map(str, unknown)),
                                                                            ", ".join(list(VALIDATION_DEFAULTS) + list(LOOP_DEFAULTS) + [BOOTSTRAP_KEY])))
    if "target_faph" not in given:
        raise ValueError("%s: target_faph is required" % key)
    v = loop_settings(key, dict(VALIDATION_DEFAULTS, **given))
    try:
        v["target_faph"] = float(v["target_faph"])
        v["windows"] = [int(w) for w in (v["windows"] if isinstance(v["windows"], (list, tuple)) else [v["windows"]])]
        v["ignore_slices_after_accept"], v["every_evals"] = int(v["ignore_slices_after_accept"]), int(v["every_evals"])
    except (TypeError, ValueError):
        raise ValueError("%s: target_faph is a number, windows a list of integers, ignore_slices_after_accept and every_evals "
                         "integers (mode: stream / non_stream)" % key) from None
    bad = [k for k, ok in (("target_faph", v["target_faph"] == v["target_faph"]),   # any number: the grid ends at cutoff 1.0, where
                           # every count is 0, so only a target below 0 is met by no window
                           ("windows", 1 <= len(v["windows"]) <= native.OP_MAX_WINDOWS and all(1 <= w <= native.OP_MAX_WINDOW for w in v["windows"])),
                           ("mode", v["mode"] in native.STREAM_MODES), ("ignore_slices_after_accept", v["ignore_slices_after_accept"] >= 0),
                           ("data_set", isinstance(v["data_set"], str) and bool(v["data_set"])),
                           ("ambient_set", isinstance(v["ambient_set"], str) and bool(v["ambient_set"])),
                           ("every_evals", v["every_evals"] >= 1)) if not ok]
    if bad:
        raise ValueError("%s: %s out of range (target_faph a number; ignore_slices_after_accept >= 0; 1..%d windows of 1..%d; every_evals >= 1; "
                         "mode stream or non_stream; data_set, ambient_set names of modes)"
                         % (key, ", ".join(bad), native.OP_MAX_WINDOWS, native.OP_MAX_WINDOW))
    if BOOTSTRAP_KEY in given:
        v[BOOTSTRAP_KEY] = bootstrap_settings(key, given[BOOTSTRAP_KEY])
    else:
        named = [config.get(k) for k in ("minimization_metric", "maximization_metric") if config.get(k) in STREAMING_BOOTSTRAP_METRICS]
        if named:
            raise ValueError("%s: the metric %s needs the %s sub-mapping (replicates, seed, confidence, block)" % (key, ", ".join(named), BOOTSTRAP_KEY))
    if int(world) > 1:
        raise ValueError("%s is not available under data parallelism (world size %d): a rank holds its shard of the validation "
                         "stores only" % (key, int(world)))
    return v


def streaming_metrics(summary):
    """The summary of one streaming validation (``operating_summary`` with ``target_faph``) -> the ``streaming_*`` metrics.
    When no window meets the target: recall 0, FRR 1, and as FAPH the closest the grid gets - the smallest FAPH at the
    largest cutoff over the usable windows -, so a minimisation towards the target keeps improving."""
    r = summary["recommended"]
    usable = np.nonzero(summary["usable"])[0]
    if r >= 0:
        c = summary["chosen"][r]
        frr, faph = float(summary["frr"][r, c]), float(summary["faph"][r, c])
        out = dict(streaming_recall=1 - frr, streaming_false_rejection_rate=frr, streaming_false_accepts_per_hour=faph,
                   streaming_cutoff=float(summary["cutoffs"][c]), streaming_window=int(summary["windows"][r]))
    else:
        out = dict(streaming_recall=0.0, streaming_false_rejection_rate=1.0,
                   streaming_false_accepts_per_hour=float(min(summary["faph"][k, -1] for k in usable)),
                   streaming_cutoff=float("nan"), streaming_window=-1)
    out.update(streaming_hours=float(summary["hours"][r if r >= 0 else usable[0]]), streaming_positives=int(summary["n_positive"]))
    if BOOTSTRAP_KEY in summary:   # ``operating_bootstrap``: the bounds.  Without a recommended point there is no fixed point: the
        # bounds at it are the point values above (recall 0, the fallback FAPH), an interval without width
        iv = summary[BOOTSTRAP_KEY]["intervals"]
        recall = iv["recall"] or (out["streaming_recall"],) * 2
        faph = iv["false_accepts_per_hour"] or (out["streaming_false_accepts_per_hour"],) * 2
        out.update(zip(STREAMING_BOOTSTRAP_METRICS, (*recall, *faph, *iv["recall_at_target"])))
    return out


class StreamingValidation:
    """What ``train.train`` does with a ``streaming_validation`` mapping: at the evaluation boundaries that are due, the
    streaming FAPH / FRR of the model's current weights at the operating point ``target_faph`` selects, added to the
    validation metrics.  A validation draws nothing from Python's or numpy's generators.  With ``quantized`` the validation
    runs the int8 model of those weights (``quantize.LoopQuantizer``; ``quantizer``: the one a quantized ``hard_negative_mining``
    already made, to be shared); creating the quantizer draws its calibration set from generator states of its own."""

    def __init__(self, settings, model, data_processor, config, writer=None, quantizer=None):
        if getattr(data_processor, "engine", None) is not getattr(model, "engine", object()) or not hasattr(data_processor, "track_windows"):
            raise ValueError("%s needs this package's Model and FeatureHandler on one engine: the tracks are windows of the stores "
                             "resident in the model's context" % VALIDATION_KEY)
        flags = getattr(model, "flags", None)
        if flags is not None and not isinstance(model.layout, InceptionLayout):
            check_evaluation_topology(flags, config["spectrogram_length"], config["stride"], [settings["mode"]])
        self.v, self.model, self.fh, self.config, self.writer = settings, model, data_processor, config, writer
        from .quantize import loop_quantizer
        self.quantizer = loop_quantizer(VALIDATION_KEY, settings, model, data_processor, config, quantizer)   # its refusals
        self.sm = None
        self.step = 0
        self.boundaries = 0
        self.last = None   # the summary of the last validation

    def due(self, is_last):
        """called once per evaluation boundary: whether a validation runs at this one (always at the last step)"""
        self.boundaries += 1
        return is_last or self.boundaries % self.v["every_evals"] == 0

    def validate(self, step):
        self.step = int(step)
        metrics, self.last = validate_streaming(self.config, self.fh, self.model, self)
        if self.writer is not None:
            self.writer.scalars(step, **metrics)
        import logging
        logging.getLogger("microwakeword_amd.train").info(
            "Step %d (" + ("streaming, int8" if self.quantizer is not None else "streaming") + "): Validation: recall = %.2f%% at %.3f false accepts per hour (target %g) with window %d and cutoff %.2f; "
            "%.3f ambient hours, %d positives", step, metrics["streaming_recall"] * 100, metrics["streaming_false_accepts_per_hour"],
            self.v["target_faph"], metrics["streaming_window"], metrics["streaming_cutoff"], metrics["streaming_hours"],
            metrics["streaming_positives"])
        if self.v.get(BOOTSTRAP_KEY):
            b = self.v[BOOTSTRAP_KEY]
            logging.getLogger("microwakeword_amd.train").info(
                "Step %d (streaming, bootstrap): %g%% percentile intervals of %d replicates (block %d): recall [%.2f%%, %.2f%%] and [%.3f, %.3f] "
                "false accepts per hour at that cutoff; recall at the target, re-selected per replicate, [%.2f%%, %.2f%%]", step,
                b["confidence"] * 100, b["replicates"], b["block"], metrics["streaming_recall_lower"] * 100, metrics["streaming_recall_upper"] * 100,
                metrics["streaming_false_accepts_per_hour_lower"], metrics["streaming_false_accepts_per_hour_upper"],
                metrics["streaming_recall_at_target_lower"] * 100, metrics["streaming_recall_at_target_upper"] * 100)
        return metrics


def validate_streaming(config, data_processor, model, state):
    """One streaming validation of ``model``'s current weights (``state``: the ``StreamingValidation`` that keeps the settings
    and the stream): the ambient tracks of ``ambient_set``, then the label-1 tracks of ``data_set``, through one native run
    from zeroed rings with the state carried from track to track (the order of ``streaming_model_roc``), one
    ``operating_summary`` and the selection at ``target_faph``.  Returns ``(streaming_* metrics, summary)``; raises ValueError
    without a positive track or a usable window.  With a quantizer (``quantized``) the run is the int8 model of the current
    weights: ``LoopQuantizer.at(state.step)``, a ``QuantizedStreamingModel`` of it in the configured mode, the same tracks."""
    v = state.v
    if getattr(state, "quantizer", None) is not None:
        try:
            q = state.quantizer.at(state.step)
        except ValueError as e:   # a non-finite calibrated range, an ADD multiplier TFLite would abort on
            raise ValueError("%s: quantized: %s" % (VALIDATION_KEY, e)) from None
        if state.sm is not None:
            state.sm.native.close()
        state.sm = QuantizedStreamingModel(q, int(config["stride"]), v["mode"], context=model)
    elif state.sm is None:
        state.sm = StreamingModel(model, int(config["stride"]), v["mode"])   # on the model's own context
    sm = state.sm
    if getattr(state, "quantizer", None) is None:
        sm.set_weights(model.get_weights())
    sm.reset()
    amb, _ = data_processor.track_windows(v["ambient_set"], sm.frames)
    pos, _ = data_processor.track_windows(v["data_set"], sm.frames, only_label=1.0)
    if pos.size == 0:
        raise ValueError("%s: %r has no positive track" % (VALIDATION_KEY, v["data_set"]))
    offsets = sm.native.run(np.concatenate([amb, pos]))
    kind = np.concatenate([np.zeros(amb.size, np.int32), np.ones(pos.size, np.int32)])
    try:
        if v.get(BOOTSTRAP_KEY):   # the summary plus the bootstrap of its operating point: the draws are a counter hash of the seed
            b = v[BOOTSTRAP_KEY]
            summary = sm.operating_bootstrap(offsets, kind, v["windows"], CUTOFFS, v["ignore_slices_after_accept"], sm.stride,
                                             config["window_step_ms"] / 1000, v["target_faph"], b["replicates"], b["seed"], b["block"],
                                             b["confidence"])
        else:
            summary = sm.operating_summary(offsets, kind, v["windows"], CUTOFFS, v["ignore_slices_after_accept"], sm.stride,
                                           config["window_step_ms"] / 1000, v["target_faph"])
    except ValueError as e:
        raise ValueError("%s: %s" % (VALIDATION_KEY, e)) from None
    return streaming_metrics(summary), summary


def detections_report(ambient, positive, cutoff, stride=1, step_s=0.02):
    """``detections.txt`` and the arrays of ``detections.npz``: ``ambient`` / ``positive`` are what ``detections`` returned
    for the ambient tracks and for the positive tracks (or None).  Lists every ambient false accept - track number, time of
    the moving-average index in seconds (index * stride * step), moving average - and every positive track whose score is
    not above the cutoff (the test of test.py:380) with the time at which it came closest."""
    ev = ambient[0] if ambient is not None else np.zeros(0, native.DETECTION_DTYPE)
    n_pos = positive[3].size if positive is not None else 0
    best = positive[2] if positive is not None else np.zeros(0, np.int64)
    score = positive[3] if positive is not None else np.zeros(0, np.float32)
    missed = np.array([t for t in range(n_pos) if not score[t] > cutoff], np.int64)
    seconds = ev["index"].astype(np.float64) * stride * step_s
    lines = ["Cutoff {:.4f}: {} ambient false accepts, {} of {} positives missed".format(float(cutoff), ev.size, missed.size, n_pos)]
    for j in range(ev.size):
        lines.append("ambient track {}: t={:.3f} s; average={:.6f}".format(int(ev["track"][j]), seconds[j], float(ev["average"][j])))
    for t in missed:
        lines.append("missed positive track {}: score={:.6f}; t={:.3f} s".format(int(t), float(score[t]), float(best[t]) * stride * step_s))
    arrays = dict(cutoff=np.float64(cutoff), ambient_track=ev["track"].copy(), ambient_index=ev["index"].copy(), ambient_seconds=seconds,
                  ambient_average=ev["average"].copy(), positive_score=np.asarray(score, np.float32),
                  positive_best_index=np.asarray(best, np.int64), missed_positive_track=missed)
    return "".join(line + "\n" for line in lines), arrays


def compute_metrics(true_positives, true_negatives, false_positives, false_negatives):
    """test.py:30-70."""
    accuracy = false_positive_rate = false_negative_rate = recall = precision = float("nan")
    count = true_positives + true_negatives + false_positives + false_negatives
    if count > 0:
        accuracy = (true_positives + true_negatives) / count
    if false_positives + true_negatives > 0:
        false_positive_rate = false_positives / (false_positives + true_negatives)
    if true_positives + false_negatives > 0:
        false_negative_rate = false_negatives / (true_positives + false_negatives)
        recall = true_positives / (true_positives + false_negatives)
    if true_positives + false_positives > 0:
        precision = true_positives / (true_positives + false_positives)
    return dict(accuracy=accuracy, recall=recall, precision=precision, false_positive_rate=false_positive_rate,
                false_negative_rate=false_negative_rate, count=count)


def metrics_to_string(m):
    """test.py:73-91."""
    return ("accuracy = {accuracy:.4%}; recall = {recall:.4%}; precision = {precision:.4%}; fpr = {fpr:.4%}; fnr = {fnr:.4%}; "
            "(N={count})").format(accuracy=m["accuracy"], recall=m["recall"], precision=m["precision"], fpr=m["false_positive_rate"],
                                  fnr=m["false_negative_rate"], count=m["count"])


def model_accuracy(config, folder, model, data_processor, data_set="testing", accuracy_name="testing_set_metrics.txt"):
    """test.py:207-290 ``tf_model_accuracy``: the non-streaming model on ``get_data(data_set, truncation_strategy=
    "truncate_start")``, p > 0.5 against the label, counted on the device (mww_evaluate_windows).  Writes
    ``<train_dir>/<folder>/<accuracy_name>`` and returns the metric dict."""
    _, _, _ = data_processor.evaluate_on_device(model, data_set, config["spectrogram_length"], "truncate_start")
    raw = model.engine.metrics_raw()
    tp, fp, fn, n = int(raw.tp5), int(raw.fp5), int(raw.fn5), int(raw.n)
    m = compute_metrics(tp, n - tp - fp - fn, fp, fn)
    path = os.path.join(config["train_dir"], folder)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, accuracy_name), "wt") as fd:
        fd.write(metrics_to_string(m))
    return m
