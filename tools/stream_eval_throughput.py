"""Throughput of the streaming evaluation (csrc/tu_stream.hip; Inception: csrc/tu_stream_graph.hip) on synthetic u16 stores: N hours of ambient tracks plus
positives through ``StreamingModel.predict_tracks`` + the metrics kernel, against the windowed alternative at the same stride
(``Engine.evaluate_windows`` over every s-th T-frame window of the ambient audio).  Prints one JSON line.

    python tools/stream_eval_throughput.py --hours 20
    python tools/stream_eval_throughput.py --hours 20 --quantized   # the int8 model (csrc/tu_stream_q8.hip); also times
                                                                    # the calibration pass (500 spectrograms) + quantization
    python tools/stream_eval_throughput.py --hours 20 --model inception   # the default Inception flags, T = 176
    python tools/stream_eval_throughput.py --hours 20 --model inception --quantized   # its int8 model (csrc/tu_stream_graph_q8.hip)
    python tools/stream_eval_throughput.py --hours 20 --residual_connection 1,0,1,0 --pooled 1   # the float kernel's <VAR> form
    python tools/stream_eval_throughput.py --hours 20 --residual_connection 1,0,1,0 --pooled 1 --quantized   # its int8 model
                                                                    # (the int8 kernel's <VAR> form, quantize_mixednet.py)
    python tools/stream_eval_throughput.py --hours 20 --mode non_stream --residual_connection 1,0,1,0 --repeat_in_block 1,2,1,1 \
        --spatial_attention 1 --pooled 1 --max_pool 1     # every window of the non-streaming model (attention: this mode only)
    python tools/stream_eval_throughput.py --hours 20 --detections 0.5 --detections_out profiles/stream_detections_throughput.txt
        # adds, on the ambient probabilities of the same session: mww_stream_metrics at the 101 cutoffs (the yardstick),
        # mww_stream_detections at the cutoff and at 0.0 (every index a candidate); medians of --detections_reps calls
    python tools/stream_eval_throughput.py --hours 20 --operating_points --operating_points_out profiles/stream_operating_points_throughput.txt
        # adds, on the same ambient probabilities: mww_stream_metrics at one window (the yardstick) against ONE
        # mww_stream_operating_points call for 10 windows x 101 cutoffs, on CUTOFFS (cutoff 0: every index a candidate) and on
        # 101 quantiles of the moving averages (every cutoff splits the indices differently)
    python tools/stream_eval_throughput.py --hours 20 --mine 2000 --mine_out profiles/stream_mine_throughput.txt
        # adds, on the same ambient probabilities: ONE mww_stream_mine call keeping MAX_NEW clips against the chain it replaces
        # (mww_stream_detections at full capacity, the host argsort, detection_clips), at cutoff 0.0 (every index a candidate)
        # and at a cutoff that leaves fewer than MAX_NEW events; byte equality is checked before anything is timed
    python tools/stream_eval_throughput.py --hours 20 --summary --summary_out profiles/stream_operating_summary_throughput.txt
        # adds, on the probabilities of the ambient tracks followed by the positives: ONE mww_stream_operating_summary call for
        # 10 windows x 101 cutoffs with the selection against the chain it replaces (mww_stream_operating_points + the host's
        # _operating_grid); equality is checked before anything is timed.  --positives 50000: the validation-sized case
    python tools/stream_eval_throughput.py --hours 1 --calibrate --calibrate_out profiles/int8_in_loop.txt
        # adds: mww_stream_calibrate over 500 windows of T - 1 rows of the resident ambient store against mww_stream_calibrate_host
        # on the host rows of the same windows (the calibration of the int8 model inside the training loop); the
        # ranges are compared first, then medians of --detections_reps calls each, from zeroed rings
    python tools/stream_eval_throughput.py --hours 20 --bootstrap 1000 --bootstrap_out profiles/stream_operating_bootstrap_throughput.txt
        # adds, on the probabilities of the ambient tracks followed by the positives: ONE StreamingModel.operating_bootstrap call
        # (the summary, mww_stream_operating_bootstrap with R replicates, the intervals) at block 0 and block 30720 against
        # operating_summary alone; the records are first compared with streaming.operating_bootstrap_host on a reduced set
        # (the restatement walks every moving-average value in Python), which is also where the restatement is timed
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microwakeword_amd import inception, mixednet, native, quantize, quantize_graph, quantize_mixednet, streaming  # noqa: E402

DEF = dict(pointwise_filters="48,48,48,48", residual_connection="0,0,0,0", repeat_in_block="1,1,1,1",
           mixconv_kernel_sizes="[5],[9],[13],[21]", max_pool=0, first_conv_filters=32, first_conv_kernel_size=3,
           spatial_attention=0, pooled=0, stride=1)
INC = dict(cnn1_filters="24", cnn1_kernel_sizes="5", cnn1_subspectral_groups="4", cnn2_filters1="10,10,16", cnn2_filters2="10,10,16",
           cnn2_kernel_sizes="5,5,5", cnn2_subspectral_groups="1,1,1", cnn2_dilation="1,1,1", dropout=0.2)   # inception.py:145-209


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=20.0)
    ap.add_argument("--track_minutes", type=float, default=60.0)
    ap.add_argument("--positives", type=int, default=2000)
    ap.add_argument("--model", choices=("mixednet", "inception"), default="mixednet")
    ap.add_argument("--frames", type=int, default=None, help="window length T (default 194 for mixednet, 176 for inception)")
    ap.add_argument("--window_hours", type=float, default=1.0, help="ambient hours the windowed alternative is timed on")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quantized", action="store_true", help="time the int8 streaming model instead of the float one")
    ap.add_argument("--mode", choices=("stream", "non_stream"), default="stream")
    for flag in ("residual_connection", "repeat_in_block"):
        ap.add_argument("--" + flag, default=DEF[flag], help="mixednet flag (default %s)" % DEF[flag])
    for flag in ("spatial_attention", "pooled", "max_pool"):
        ap.add_argument("--" + flag, type=int, default=0, help="mixednet flag")
    ap.add_argument("--detections", type=float, default=None, metavar="CUTOFF",
                    help="also time mww_stream_detections at this cutoff and at 0.0 against mww_stream_metrics on the ambient probabilities")
    ap.add_argument("--detections_reps", type=int, default=15)
    ap.add_argument("--detections_out", default=None, help="write the detection leg's times and event counts to this text file")
    ap.add_argument("--operating_points", action="store_true",
                    help="also time one mww_stream_operating_points call (10 windows x 101 cutoffs) against mww_stream_metrics at one window")
    ap.add_argument("--operating_points_out", default=None, help="write the operating-point leg's times and scratch size to this text file")
    ap.add_argument("--mine", type=int, default=None, metavar="MAX_NEW",
                    help="also time mww_stream_mine keeping MAX_NEW clips against mww_stream_detections + argsort + detection_clips")
    ap.add_argument("--mine_out", default=None, help="write the mining leg's times and read-back sizes to this text file")
    ap.add_argument("--summary", action="store_true",
                    help="also time one mww_stream_operating_summary call (10 windows x 101 cutoffs) against mww_stream_operating_points + the host grid")
    ap.add_argument("--summary_out", default=None, help="append the summary leg's times, read-back and scratch sizes to this text file")
    ap.add_argument("--summary_target", type=float, default=0.5, help="target FAPH of the summary leg's selection")
    ap.add_argument("--bootstrap", type=int, default=None, metavar="R",
                    help="also time one StreamingModel.operating_bootstrap call with R replicates (block 0 and 30720) against operating_summary alone")
    ap.add_argument("--bootstrap_out", default=None, help="append the bootstrap leg's times and read-back sizes to this text file")
    ap.add_argument("--calibrate", action="store_true",
                    help="also time mww_stream_calibrate over 500 resident windows against mww_stream_calibrate_host on their host rows")
    ap.add_argument("--calibrate_out", default=None, help="append the calibration leg's times to this text file")
    a = ap.parse_args()
    if a.model == "inception":
        T = a.frames or 176
        model = inception.model(INC, (T, 40), 1024, max_batch=1024, seed=3)
        name = "inception cnn1 %s/%s/%s cnn2 %s/%s k %s d %s (T=%d)" % (
            INC["cnn1_filters"], INC["cnn1_kernel_sizes"], INC["cnn1_subspectral_groups"], INC["cnn2_filters1"], INC["cnn2_filters2"],
            INC["cnn2_kernel_sizes"], INC["cnn2_dilation"], T)
    else:
        T = a.frames or 194
        flags = dict(DEF, residual_connection=a.residual_connection, repeat_in_block=a.repeat_in_block,
                     spatial_attention=a.spatial_attention, pooled=a.pooled, max_pool=a.max_pool)
        model = mixednet.model(flags, (T, 40), 1024, max_batch=1024, seed=3)
        changed = ["%s=%s" % (k, v) for k, v in flags.items() if v != DEF[k]]
        name = "mixednet default%s (T=%d)" % ("".join(" " + c for c in changed), T)
    rng = np.random.default_rng(0)
    per_track = int(a.track_minutes * 60 * 50)
    n_amb = max(1, int(round(a.hours * 60 / a.track_minutes)))
    amb_frames = per_track * n_amb
    amb = rng.integers(0, 1000, size=(amb_frames, 40), dtype=np.uint16)
    pos_len = rng.integers(80, 150, a.positives)
    pos = rng.integers(0, 1000, size=(int(pos_len.sum()), 40), dtype=np.uint16)
    model.engine.upload_store(0, amb.reshape(-1))
    model.engine.upload_store(1, pos.reshape(-1))
    amb_win = np.zeros(n_amb, native.WINDOW_DTYPE)
    amb_win["store"], amb_win["copy_rows"], amb_win["src_elem"] = 0, per_track, np.arange(n_amb, dtype=np.int64) * per_track * 40
    pos_win = np.zeros(a.positives, native.WINDOW_DTYPE)
    pos_off = np.concatenate([[0], np.cumsum(pos_len)[:-1]]).astype(np.int64)
    pos_win["store"], pos_win["pad_rows"] = 1, np.maximum(0, T - pos_len)
    pos_win["copy_rows"], pos_win["src_elem"] = pos_len, pos_off * 40
    sm = streaming.StreamingModel(model, 1, a.mode)
    extra = {} if a.mode == "stream" else {"mode": a.mode}
    if a.quantized:
        # the calibration pass of --test_tflite_streaming_quantized: 500 spectrograms of T frames, chunks of s = 1
        cal = rng.integers(0, 1000, size=(quantize.CALIBRATION_SAMPLES * (T - 1), 40)).astype(np.float32) * streaming.SCALE_U16
        if a.model == "inception":   # the graph stream that takes the int8 calls, and the graph contract
            desc = streaming.graph_stream_description(INC, T, 1, "stream")
            flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()])

            def calibration_stream():
                st = native.GraphStream(model.engine, desc, int8=True)
                st.set_weights(flat)
                return st
            q = quantize_graph
        elif streaming.mixednet_variant_flags(flags):   # residual / pooled: the stream that takes the int8 calls, and its contract
            desc = streaming.mixednet_stream_description(flags, T, 1, "stream")
            flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()])

            def calibration_stream():
                st = native.Stream(model.engine, desc, int8=True)
                st.set_weights(flat)
                return st
            q = quantize_mixednet
        else:
            calibration_stream = lambda: streaming.StreamingModel(model, 1, "stream").native   # noqa: E731
            q = quantize
        calibration_stream().calibrate_host(cal[:1000])   # warm-up
        cs = []
        for _ in range(a.reps):
            c = calibration_stream()
            t0 = time.perf_counter()
            ranges = c.calibrate_host(cal)
            qm = q.quantize(model, ranges)
            cs.append(time.perf_counter() - t0)
        sm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
        extra = {"quantized": "int8", "calibration_frames": int(cal.shape[0]), "calibration_seconds": round(min(cs), 4)}

    def once():
        off = sm.native.run(amb_win)
        sm.metrics(off, np.zeros(n_amb, np.int32))
        n = int(off[-1])
        off = sm.native.run(pos_win)
        sm.metrics(off, np.ones(a.positives, np.int32))
        return n + int(off[-1])

    once()   # warm-up
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        n_out = once()
        ts.append(time.perf_counter() - t0)
    t = min(ts)
    hours = (amb_frames + int(pos_len.sum())) * 0.02 / 3600
    # windowed alternative: every 1-frame-stride T-frame window of `window_hours` of the ambient audio
    nw = int(a.window_hours * 3600 * 50)
    nw = min(nw, amb_frames - T)
    win = np.zeros(nw, native.WINDOW_DTYPE)
    win["store"], win["copy_rows"], win["src_elem"] = 0, T, np.arange(nw, dtype=np.int64) * 40
    labels = np.zeros(nw, np.float32)
    model.engine.evaluate_windows(win[:4096], labels[:4096], 1024)
    model.engine.synchronize()
    t0 = time.perf_counter()
    model.engine.evaluate_windows(win, labels, 1024)
    model.engine.synchronize()
    tw = time.perf_counter() - t0
    rec = {"tool": "stream_eval_throughput", "model": name, **extra, "stride": 1, "ambient_hours": round(amb_frames * 0.02 / 3600, 3),
           "ambient_tracks": n_amb, "positives": a.positives, "outputs": n_out, "seconds": round(t, 4),
           "outputs_per_s": round(n_out / t, 1), "audio_hours_per_s": round(hours / t, 3),
           "windowed_outputs": nw, "windowed_seconds": round(tw, 4), "windowed_outputs_per_s": round(nw / tw, 1),
           "speedup_vs_windowed": round((n_out / t) / (nw / tw), 2), "library": model.engine.nl.version()}
    if a.detections is not None:
        rec["detections"] = detections_leg(sm, amb_win, a.detections, a.detections_reps)
        if a.detections_out:
            with open(a.detections_out, "wt") as fd:
                fd.write(detections_text(rec))
    if a.operating_points:
        rec["operating_points"] = operating_points_leg(sm, amb_win, a.detections_reps)
        if a.operating_points_out:
            with open(a.operating_points_out, "wt") as fd:
                fd.write(operating_points_text(rec))
    if a.mine is not None:
        rec["mine"] = mine_leg(sm, amb_win, a.mine, a.detections_reps)
        if a.mine_out:
            with open(a.mine_out, "wt") as fd:
                fd.write(mine_text(rec))
    if a.summary:
        rec["summary"] = summary_leg(sm, amb_win, pos_win, a.detections_reps, a.summary_target)
        if a.summary_out:
            with open(a.summary_out, "at") as fd:
                fd.write(summary_text(rec))
    if a.bootstrap is not None:
        rec["bootstrap"] = bootstrap_leg(sm, amb_win, pos_win, a.bootstrap, a.detections_reps, a.summary_target)
        if a.bootstrap_out:
            with open(a.bootstrap_out, "at") as fd:
                fd.write(bootstrap_text(rec))
    if a.calibrate:
        rec["calibrate"] = calibrate_leg(model, a.model, amb, T, a.detections_reps)
        if a.calibrate_out:
            with open(a.calibrate_out, "at") as fd:
                fd.write(calibrate_text(rec))
    print(json.dumps(rec), flush=True)


def calibrate_leg(model, kind, amb, T, reps, samples=quantize.CALIBRATION_SAMPLES):
    """``samples`` windows of T - 1 rows (what calibration_windows leaves of a T-row draw at stride 1) at random rows of the
    resident ambient store, a tenth of them padded in front: ONE mww_stream_calibrate call against ONE mww_stream_calibrate_host
    call on the host rows of the same windows, each on a stream of its own, from zeroed rings"""
    rng = np.random.default_rng(7)
    win = np.zeros(samples, native.WINDOW_DTYPE)
    pad = np.where(rng.random(samples) < 0.1, rng.integers(1, T - 1, samples), 0)
    win["store"], win["pad_rows"], win["copy_rows"] = 0, pad, T - 1 - pad
    win["src_elem"] = rng.integers(0, amb.shape[0] - T, samples).astype(np.int64) * 40
    rows = np.concatenate([np.concatenate([np.zeros((int(w["pad_rows"]), 40), np.float32),
                                           amb[int(w["src_elem"]) // 40:int(w["src_elem"]) // 40 + int(w["copy_rows"])].astype(np.float32)
                                           * streaming.SCALE_U16]) for w in win])
    flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()])

    def stream():
        if kind == "inception":
            st = native.GraphStream(model.engine, streaming.graph_stream_description(model.flags, T, 1, "stream"), int8=True)
        elif streaming.mixednet_variant_flags(model.flags):
            st = native.Stream(model.engine, streaming.mixednet_stream_description(model.flags, T, 1, "stream"), int8=True)
        else:
            return streaming.StreamingModel(model, 1, "stream").native
        st.set_weights(flat)
        return st
    dev, host = stream(), stream()
    _, got = dev.calibrate(win)
    want = host.calibrate_host(rows)
    assert np.array_equal(got, want), "mww_stream_calibrate differs from mww_stream_calibrate_host"
    assert dev.read().tobytes() == host.read().tobytes()
    out = {"windows": int(samples), "frames": int(rows.shape[0]), "tensors": int(got.shape[0]), "reps": int(reps),
           "host_bytes_up": int(rows.nbytes), "device_bytes_back": int(got.nbytes)}
    for name, st, call in (("calibrate_ms", dev, lambda: dev.calibrate(win)), ("calibrate_host_ms", host, lambda: host.calibrate_host(rows))):
        ts = []
        for _ in range(reps + 1):   # (the first call is the warm-up)
            st.reset()
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        out[name] = round(1e3 * float(np.median(ts[1:])), 3)
    out["ratio"] = round(out["calibrate_ms"] / out["calibrate_host_ms"], 4)
    return out


def calibrate_text(rec):
    d = rec["calibrate"]
    return "\n".join([
        "mww_stream_calibrate against mww_stream_calibrate_host, one session (tools/stream_eval_throughput.py --calibrate)",
        "%s, %s" % (rec["model"], rec["library"]),
        "%d windows, %d frames, %d tensors; ranges and probabilities equal; medians of %d calls after a warm-up, from zeroed rings"
        % (d["windows"], d["frames"], d["tensors"], d["reps"]),
        "  mww_stream_calibrate_host (host rows):     %9.3f ms, %9d bytes uploaded" % (d["calibrate_host_ms"], d["host_bytes_up"]),
        "  mww_stream_calibrate (resident windows):   %9.3f ms, %9d bytes read back" % (d["calibrate_ms"], d["device_bytes_back"]),
        "  ratio window form / host form:             %9.4f" % d["ratio"], ""]) + "\n"


def summary_leg(sm, amb_win, pos_win, reps, target, cooldown=25, step_s=0.02):
    """One session, the probabilities of the ambient tracks followed by the positives (one native run): the median wall time of
    `reps` calls (after one warm-up call each) of ONE StreamingModel.operating_summary call - windows 1..10 x the 101 cutoffs,
    the selection at `target` included - and of the chain it replaces: mww_stream_operating_points, then the host's
    _operating_grid (track_hours, false_rejection_rates, select_operating_points).  Counts, hours, usable, FAPH, FRR and the
    selection are compared bit for bit before anything is timed.  Bytes: what each side copies from the device, and the device
    memory each call needs next to the transfer tables (both from the sizes)."""
    n_amb, n_pos = int(amb_win.size), int(pos_win.size)
    off = sm.native.run(np.concatenate([amb_win, pos_win]))
    kind = np.concatenate([np.zeros(n_amb, np.int32), np.ones(n_pos, np.int32)])
    windows, cut = streaming.OP_WINDOWS, streaming.CUTOFFS
    W, C, n = len(windows), cut.size, n_amb + n_pos

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3)

    def chain():
        counts, ma_len, score = sm.operating_points(off, kind, windows, cut, cooldown)
        return streaming._operating_grid(counts, ma_len[:, :n_amb], ma_len[:, n_amb:], score[:, n_amb:], windows, cut, sm.stride, step_s, target)

    def call():
        return sm.operating_summary(off, kind, windows, cut, cooldown, sm.stride, step_s, target)

    want, got = chain(), call()
    for k in ("counts", "hours", "usable", "faph", "frr", "chosen", "chosen_cutoff"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert got["recommended"] == want["recommended"] and got["n_positive"] == n_pos and got["usable"].all()
    lengths = np.diff(off) - np.where(kind == 1, cooldown, 0)
    n_seg = int(sum((max(int(m) - min(windows) + 1, 0) + 1023) // 1024 for m in lengths))
    ma = np.maximum(lengths - min(windows) + 1, 0)
    tables, tables_ambient = operating_points_scratch(ma, W, C, cooldown), operating_points_scratch(ma[:n_amb], W, C, cooldown)
    n_blk = (n_pos + 255) // 256
    r = got["recommended"]
    return {"probabilities": int(off[-1]), "ambient_tracks": n_amb, "positives": n_pos, "reps": reps, "windows": list(windows),
            "cooldown": cooldown, "target_faph": target, "recommended_window": int(windows[r]) if r >= 0 else None,
            "chain_ms": median_ms(chain), "grid_call_ms": median_ms(lambda: sm.operating_points(off, kind, windows, cut, cooldown)),
            "summary_ms": median_ms(call),
            "chain_bytes": W * C * 8 + W * n * 12, "summary_bytes": W * C * 16 + W * 24 + 16,
            "chain_table_bytes": tables, "summary_table_bytes": tables_ambient,
            "chain_scratch_bytes": W * C * 8 + W * n * 12 + W * n * C * 8 + W * n_seg * 4,
            "summary_scratch_bytes": W * C * 16 + W * 24 + 16 + W * n_amb * C * 8 + W * n_blk * (C + 1) * 4 + W * n_seg * 4}


def bootstrap_leg(sm, amb_win, pos_win, replicates, reps, target, cooldown=25, step_s=0.02, blocks=(0, 30720), check=(2, 40000, 200, 64)):
    """One session.  First the check, on a reduced set - `check` = (ambient tracks, rows kept of each, positives, replicates):
    the restatement walks every moving-average value in Python, some 10 us per value and window -: the dict of
    StreamingModel.operating_bootstrap against streaming.operating_bootstrap_host on the probabilities read back, records and
    intervals byte for byte, at each block; the restatement's wall time there is recorded next to the device call's.  Then, on
    the probabilities of all ambient tracks followed by the positives (one native run): the median wall time of `reps` calls
    (after one warm-up call each) of operating_summary alone and of operating_bootstrap with `replicates` replicates at each
    block - the summary, mww_stream_operating_bootstrap, the intervals; host work included."""
    windows, cut = streaming.OP_WINDOWS, streaming.CUTOFFS

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3)

    c_amb, c_rows, c_pos, c_rep = check
    small = amb_win[:c_amb].copy()
    small["copy_rows"] = np.minimum(small["copy_rows"], c_rows)
    sm.reset()
    off = sm.native.run(np.concatenate([small, pos_win[:c_pos]]))
    kind = np.concatenate([np.zeros(small.size, np.int32), np.ones(min(c_pos, pos_win.size), np.int32)])
    p = sm.read_probabilities()
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    out = {"replicates": int(replicates), "reps": reps, "windows": list(windows), "cooldown": cooldown, "target_faph": target,
           "record_bytes": native.BOOT_RECORD_DTYPE.itemsize,
           "check": {"ambient_tracks": int(small.size), "positives": int(kind.sum()), "probabilities": int(off[-1]), "replicates": c_rep}}
    for block in blocks:
        t0 = time.perf_counter()
        want = streaming.operating_bootstrap_host(tracks[:small.size], tracks[small.size:], windows, cut, sm.stride, step_s, cooldown, target,
                                                  c_rep, 1, block)
        host_s = time.perf_counter() - t0
        got = sm.operating_bootstrap(off, kind, windows, cut, cooldown, sm.stride, step_s, target, c_rep, 1, block)
        assert got["bootstrap"]["records"].tobytes() == want["bootstrap"]["records"].tobytes(), block
        assert got["bootstrap"]["intervals"] == want["bootstrap"]["intervals"] and got["recommended"] == want["recommended"], block
        for k in ("counts", "accepts", "hours", "faph", "frr", "chosen"):
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (block, k)
        out["check"]["block_%d" % block] = {"host_restatement_s": round(host_s, 3),
                                            "device_ms": median_ms(lambda: sm.operating_bootstrap(off, kind, windows, cut, cooldown, sm.stride, step_s,
                                                                                                  target, c_rep, 1, block))}
    n_amb, n_pos = int(amb_win.size), int(pos_win.size)
    sm.reset()
    off = sm.native.run(np.concatenate([amb_win, pos_win]))
    kind = np.concatenate([np.zeros(n_amb, np.int32), np.ones(n_pos, np.int32)])
    W, C = len(windows), cut.size
    out.update(probabilities=int(off[-1]), ambient_tracks=n_amb, positives=n_pos, read_back_bytes=replicates * native.BOOT_RECORD_DTYPE.itemsize,
               summary_ms=median_ms(lambda: sm.operating_summary(off, kind, windows, cut, cooldown, sm.stride, step_s, target)),
               summary_bytes=W * C * 16 + W * 24 + 16)
    for block in blocks:
        g = sm.operating_bootstrap(off, kind, windows, cut, cooldown, sm.stride, step_s, target, replicates, 1, block)
        again = sm.operating_bootstrap(off, kind, windows, cut, cooldown, sm.stride, step_s, target, replicates, 1, block)
        assert g["bootstrap"]["records"].tobytes() == again["bootstrap"]["records"].tobytes()
        n_blk = int(sum(-(-int(n) // block) if block else 1 for n in np.diff(off)[:n_amb]))
        out["block_%d" % block] = {
            "blocks": n_blk, "scratch_bytes": W * n_blk * C * 4 + W * n_blk * 8 + W * n_pos,
            "bootstrap_ms": median_ms(lambda: sm.operating_bootstrap(off, kind, windows, cut, cooldown, sm.stride, step_s, target, replicates, 1, block)),
            "native_call_ms": median_ms(lambda: sm.native.operating_bootstrap(off, kind, windows, cut, cooldown, cooldown, sm.stride, step_s, target,
                                                                              replicates, 1, block, None)),
            "intervals": g["bootstrap"]["intervals"], "replicates_without_point": int(np.count_nonzero(g["bootstrap"]["records"]["sel_row"] < 0))}
    return out


def bootstrap_text(rec):
    d = rec["bootstrap"]
    c = d["check"]
    lines = ["StreamingModel.operating_bootstrap against operating_summary alone, one session (tools/stream_eval_throughput.py --bootstrap %d --positives %d)"
             % (d["replicates"], d["positives"]),
             "library: %s" % rec["library"], "model: %s%s" % (rec["model"], ", int8" if rec.get("quantized") else ""),
             "check first, on %d probabilities (%d ambient tracks + %d positives), %d replicates: records, intervals, summary byte-identical to "
             "streaming.operating_bootstrap_host" % (c["probabilities"], c["ambient_tracks"], c["positives"], c["replicates"])]
    for name in sorted(k for k in c if k.startswith("block_")):
        lines.append("  %-12s the restatement %9.3f s (one run), the device call %9.3f ms" % (name.replace("_", " ") + ":", c[name]["host_restatement_s"], c[name]["device_ms"]))
    lines += ["%d probabilities: %d ambient tracks + %d positives, windows %s x 101 cutoffs, cooldown %d, target %g FAPH, %d replicates; median wall "
              "time of %d calls each after a warm-up call, host work included"
              % (d["probabilities"], d["ambient_tracks"], d["positives"], ",".join(str(w) for w in d["windows"]), d["cooldown"], d["target_faph"],
                 d["replicates"], d["reps"]),
              "  operating_summary alone:                          %10.3f ms, %9d bytes read back" % (d["summary_ms"], d["summary_bytes"])]
    for name in sorted((k for k in d if k.startswith("block_")), key=lambda k: int(k.split("_")[1])):
        b = d[name]
        lines.append("  operating_bootstrap, %-12s %5d blocks:   %10.3f ms (mww_stream_operating_bootstrap alone %.3f ms), %9d + %d bytes read back, "
                     "%d bytes of block tables" % (name.replace("_", " ") + ",", b["blocks"], b["bootstrap_ms"], b["native_call_ms"], d["summary_bytes"],
                                                   d["read_back_bytes"], b["scratch_bytes"]))
        lines.append("      intervals %s; %d replicates without a point" % (json.dumps(b["intervals"]), b["replicates_without_point"]))
    lines.append("")
    return "".join(line + "\n" for line in lines)


def summary_text(rec):
    d = rec["summary"]
    lines = ["mww_stream_operating_summary against the chain it replaces, one session (tools/stream_eval_throughput.py --summary --positives %d)"
             % d["positives"],
             "library: %s" % rec["library"], "model: %s%s" % (rec["model"], ", int8" if rec.get("quantized") else ""),
             "%d probabilities: %d ambient tracks + %d positives, windows %s x 101 cutoffs, cooldown %d, target %g FAPH; median wall time "
             "of %d calls each, host work included; counts, hours, FAPH, FRR and the selection bit-identical on both sides"
             % (d["probabilities"], d["ambient_tracks"], d["positives"], ",".join(str(w) for w in d["windows"]), d["cooldown"],
                d["target_faph"], d["reps"]),
             "  mww_stream_operating_points + _operating_grid on the host: %10.3f ms (the call alone %.3f ms), %10d bytes read back, %11d bytes of device scratch"
             % (d["chain_ms"], d["grid_call_ms"], d["chain_bytes"], d["chain_scratch_bytes"]),
             "  mww_stream_operating_summary + the selection:              %10.3f ms, %31d bytes read back, %11d bytes of device scratch"
             % (d["summary_ms"], d["summary_bytes"], d["summary_scratch_bytes"]),
             "  transfer tables resident at a time: %d bytes (a row per segment) against %d bytes (the ambient segments alone)"
             % (d["chain_table_bytes"], d["summary_table_bytes"]),
             "the bar: summary <= chain: %s" % ("met" if d["summary_ms"] <= d["chain_ms"] else "MISSED"), ""]
    return "".join(line + "\n" for line in lines)


def detections_leg(sm, amb_win, cutoff, reps):
    """One session, the same ambient probabilities: the median wall time of `reps` calls (after one warm-up call each) of
    mww_stream_metrics at the 101 cutoffs and of mww_stream_detections (one call, capacity = the count) at `cutoff`, at
    0.0 and at the median moving average, window 5, cooldown 25."""
    off = sm.native.run(amb_win)
    kind = np.zeros(amb_win.size, np.int32)

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3)

    out = {"probabilities": int(off[-1]), "tracks": int(amb_win.size), "reps": reps, "window": 5, "cooldown": 25,
           "metrics_101_cutoffs_ms": median_ms(lambda: sm.metrics(off, kind))}
    counts, _, _ = sm.metrics(off, kind)
    # a model with random weights may put every probability on one side of `cutoff`: the median of the moving averages makes
    # about half of the indices candidates
    p = sm.read_probabilities()
    med = float(np.median(np.concatenate([streaming.moving_average_in_order(p[off[t]:off[t + 1]], 5) for t in range(amb_win.size)])))
    for name, c in (("cutoff", float(cutoff)), ("worst_case", 0.0), ("median", med)):
        events, track_count, _, _ = sm.detections(off, kind, c)
        n = int(track_count.sum())
        at = int(np.argmin(np.abs(streaming.CUTOFFS - c)))
        assert events.size == n and (abs(streaming.CUTOFFS[at] - c) > 1e-9 or n == int(counts[at])), (n, counts[at])
        out[name] = {"cutoff": c, "events": n,
                     "detections_ms": median_ms(lambda: sm.native.detections(off, kind, c, 5, 25, 25, capacity=n)),
                     "count_only_ms": median_ms(lambda: sm.native.detections(off, kind, c, 5, 25, 25, capacity=0))}
    return out


def operating_points_scratch(ma_lengths, n_windows, n_cutoffs, cooldown, seg=1024, budget=96 << 20):
    """bytes of transfer tables resident at a time (ma_lengths: per track, at the smallest window)"""
    n_seg = sum((int(m) + seg - 1) // seg for m in ma_lengths)
    per_window = max(n_seg, 1) * min(max(cooldown, 1), seg) * n_cutoffs * 4
    return per_window * min(n_windows, max(budget // per_window, 1))


def operating_points_leg(sm, amb_win, reps, cooldown=25):
    """One session, the same ambient probabilities: the median wall time of `reps` calls (after one warm-up call each) of
    mww_stream_metrics at the 101 cutoffs and window 5 (the yardstick) and of one mww_stream_operating_points call for windows
    1..10 at the 101 cutoffs of CUTOFFS (0.0 among them: every index a candidate) and at 101 quantiles of the window-5
    moving averages; host round trips included.  Every row is checked against the metrics call of its window."""
    off = sm.native.run(amb_win)
    kind = np.zeros(amb_win.size, np.int32)
    windows = streaming.OP_WINDOWS

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3)

    p = sm.read_probabilities()
    mas = np.concatenate([streaming.moving_average_in_order(p[off[t]:off[t + 1]], 5) for t in range(amb_win.size)])
    quantiles = np.quantile(mas.astype(np.float64), np.linspace(0, 1, streaming.CUTOFFS.size))
    out = {"probabilities": int(off[-1]), "tracks": int(amb_win.size), "reps": reps, "windows": list(windows), "cooldown": cooldown,
           "scratch_bytes": operating_points_scratch(np.diff(off) - min(windows) + 1, len(windows), streaming.CUTOFFS.size, cooldown)}
    for name, cut in (("cutoffs", streaming.CUTOFFS), ("quantiles", quantiles)):
        counts, ma_len, _ = sm.operating_points(off, kind, windows, cut, cooldown)
        for k, w in enumerate(windows):
            m = sm.metrics(off, kind, cut, w, cooldown)
            assert np.array_equal(counts[k], m[0]) and np.array_equal(ma_len[k], m[1]), (name, w)
        out[name] = {"metrics_one_window_ms": median_ms(lambda: sm.metrics(off, kind, cut, 5, cooldown)),
                     "grid_ms": median_ms(lambda: sm.operating_points(off, kind, windows, cut, cooldown)),
                     "false_accepts_window_5": [int(counts[4, 0]), int(counts[4, cut.size // 2]), int(counts[4, -1])]}
    return out


def operating_points_text(rec):
    d = rec["operating_points"]
    lines = ["mww_stream_operating_points against mww_stream_metrics, one session (tools/stream_eval_throughput.py --operating_points)",
             "library: %s" % rec["library"], "model: %s%s" % (rec["model"], ", int8" if rec.get("quantized") else ""),
             "%d probabilities in %d ambient tracks (%.1f h at 20 ms), cooldown %d; median wall time of %d calls each, host round trips included"
             % (d["probabilities"], d["tracks"], d["probabilities"] * 0.02 / 3600, d["cooldown"], d["reps"]),
             "grid: windows %s x 101 cutoffs in one call; transfer tables resident: %d bytes (%.1f MB)"
             % (",".join(str(w) for w in d["windows"]), d["scratch_bytes"], d["scratch_bytes"] / 1e6)]
    for name, what in (("cutoffs", "cutoffs 0.00 .. 1.00 (0.00: every index a candidate)"), ("quantiles", "cutoffs = 101 quantiles of the moving averages")):
        c = d[name]
        lines.append("%s:" % what)
        lines.append("  mww_stream_metrics, window 5 (the yardstick):      %9.3f ms" % c["metrics_one_window_ms"])
        lines.append("  mww_stream_operating_points, 10 windows:           %9.3f ms  (false accepts at window 5, first / middle / last cutoff: %s)"
                     % (c["grid_ms"], " / ".join(str(v) for v in c["false_accepts_window_5"])))
    return "".join(line + "\n" for line in lines)


def mine_leg(sm, amb_win, max_new, reps, window=5, cooldown=25):
    """One session, the same ambient probabilities: the median wall time of `reps` calls (after one warm-up call each) of ONE
    mww_stream_mine call keeping `max_new` clips and of the chain it replaces - mww_stream_detections at full capacity (the
    count known: one call), the stable host argsort, streaming.detection_clips - at cutoff 0.0 (every index a candidate) and at
    a cutoff that leaves fewer than `max_new` events.  Clips and events are compared byte for byte before anything is timed.
    The bytes are what each side copies from the device: events (24 B) and per-track results for the chain; the kept clips
    and events (24 B each, three 256-B-aligned blocks) and the per-track counts for the call."""
    off = sm.native.run(amb_win)
    n_trk = int(amb_win.size)
    kind = np.zeros(n_trk, np.int32)

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3)

    def chain(c, n):
        events, _, _, _ = sm.native.detections(off, kind, c, window, cooldown, cooldown, capacity=n)
        if events.size > max_new:
            best = np.argsort(-events["average"].astype(np.float64), kind="stable")[:max_new]
            events = events[np.sort(best)]
        clips, kept = streaming.detection_clips(amb_win, events, sm.frames, sm.stride, sm.mode, window, return_kept=True)
        return clips, events[kept]

    p = sm.read_probabilities()
    mas = np.concatenate([streaming.moving_average_in_order(p[off[t]:off[t + 1]], window) for t in range(n_trk)])
    few = float(np.sort(mas)[-max(max_new // 2, 2)])   # at most max_new / 2 - 1 values lie above it
    al = lambda b: (b + 255) & ~255   # noqa: E731
    out = {"probabilities": int(off[-1]), "tracks": n_trk, "reps": reps, "window": window, "cooldown": cooldown, "max_new": int(max_new)}
    for name, c in (("all_candidates", 0.0), ("few_events", few)):
        _, track_count, _, _ = sm.native.detections(off, kind, c, window, cooldown, cooldown, capacity=0)
        n = int(track_count.sum())
        want_clips, want_events = chain(c, n)
        clips, events, total, counts = sm.native.mine(amb_win, off, c, window, cooldown, 0, 0, max_new)
        assert clips.tobytes() == want_clips.tobytes() and events.tobytes() == want_events.tobytes(), name
        assert total == n and np.array_equal(counts, track_count), name
        k = min(n, max_new)
        out[name] = {"cutoff": c, "events": n, "clips": int(clips.size),
                     "chain_ms": median_ms(lambda: chain(c, n)),
                     "mine_ms": median_ms(lambda: sm.native.mine(amb_win, off, c, window, cooldown, 0, 0, max_new)),
                     "chain_bytes": 8 + n * 24 + n_trk * 20,
                     "mine_bytes": 8 + n_trk * 8 + (al(al(8) + al(k * 24) + k * 24) if k else 0)}
    assert out["all_candidates"]["events"] > max_new > out["few_events"]["events"], out
    return out


def mine_text(rec):
    d = rec["mine"]
    lines = ["mww_stream_mine against the chain it replaces, one session (tools/stream_eval_throughput.py --mine %d)" % d["max_new"],
             "library: %s" % rec["library"], "model: %s%s" % (rec["model"], ", int8" if rec.get("quantized") else ""),
             "%d probabilities in %d ambient tracks (%.1f h at 20 ms), window %d, cooldown %d, max_new %d; median wall time of %d calls each, "
             "host work included; clips and events byte-identical on both sides"
             % (d["probabilities"], d["tracks"], d["probabilities"] * 0.02 / 3600, d["window"], d["cooldown"], d["max_new"], d["reps"])]
    for name, what in (("all_candidates", "every index a candidate"), ("few_events", "fewer than max_new events")):
        c = d[name]
        lines.append("cutoff %.6f (%s): %d events, %d clips kept" % (c["cutoff"], what, c["events"], c["clips"]))
        lines.append("  mww_stream_detections + argsort + detection_clips: %9.3f ms, %9d bytes read back" % (c["chain_ms"], c["chain_bytes"]))
        lines.append("  mww_stream_mine:                                    %9.3f ms, %9d bytes read back (1/%.1f)"
                     % (c["mine_ms"], c["mine_bytes"], c["chain_bytes"] / c["mine_bytes"]))
    a = d["all_candidates"]
    lines.append("the bar (all candidates): mine <= chain: %s; read-back <= 1/20 of the chain's: %s"
                 % ("met" if a["mine_ms"] <= a["chain_ms"] else "MISSED", "met" if 20 * a["mine_bytes"] <= a["chain_bytes"] else "MISSED"))
    return "".join(line + "\n" for line in lines)


def detections_text(rec):
    d = rec["detections"]
    lines = ["mww_stream_detections against mww_stream_metrics, one session (tools/stream_eval_throughput.py --detections)",
             "library: %s" % rec["library"], "model: %s%s" % (rec["model"], ", int8" if rec.get("quantized") else ""),
             "%d probabilities in %d ambient tracks (%.1f h at 20 ms), window %d, cooldown %d; median wall time of %d calls each"
             % (d["probabilities"], d["tracks"], d["probabilities"] * 0.02 / 3600, d["window"], d["cooldown"], d["reps"]),
             "mww_stream_metrics, 101 cutoffs:          %9.3f ms" % d["metrics_101_cutoffs_ms"]]
    for name in ("cutoff", "worst_case", "median"):
        c = d[name]
        lines.append("mww_stream_detections, cutoff %.4f:      %9.3f ms  (%d events; counting only, capacity 0: %.3f ms)"
                     % (c["cutoff"], c["detections_ms"], c["events"], c["count_only_ms"]))
    return "".join(line + "\n" for line in lines)


if __name__ == "__main__":
    main()
