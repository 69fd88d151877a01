"""Checks of mww_stream_mine (csrc/tu_stream_mine.hip), mining.mine_hard_negatives_on_device, FeatureHandler.set_mined_clips and
the ``hard_negative_mining`` option of train.train, shared by the emulator tests (tests/test_stream_mine_emulated.py) and the
GPU tests (tests/test_stream_mine_gpu.py): the same shapes on both.  Everything is byte equality against the chain the call
replaces: ``streaming.detection_positions`` on the in-order float32 moving average -> stable ``argsort`` ->
``streaming.detection_clips``, and ``mww_stream_detections`` for the counts."""
import json
import os
import random

import numpy as np
import pytest

from microwakeword_amd import mining, native, streaming
from microwakeword_amd.data import FeatureHandler
import engine_checks as ec
import mining_checks as mc
import stream_detect_checks as dc
import stream_sweep as ss
import streaming_checks as sc

SEG = dc.SEG          # moving-average values per detect segment (POST_SEG)
W_MAX = 5
# moving-average counts at window 5: 0, 0 (length = window - 1), 1, both sides of a segment boundary, several workgroups of events
LENGTHS = [0, W_MAX - 1, W_MAX, SEG - 1 + W_MAX - 1, SEG + W_MAX - 1, SEG + 1 + W_MAX - 1, 3001, 700, 700]
ALL_EQUAL, NEG_ZERO = 7, 8   # tracks of LENGTHS


def kernel_case(lib, stride, mode):
    """a small stream of the given stride and mode in the shared context, tracks that are windows of one uploaded store, and
    probabilities that are multiples of 1/8"""
    model = sc.context_model(lib)
    desc = dict(ss.desc_of(4, 3, stride, [(1, (3,), 8)], 2), mode=mode)
    st = native.Stream(model.engine, desc)
    frames = int(desc["frames"])
    rng = np.random.default_rng(5)
    store_rows = 900
    model.engine.upload_store(0, np.zeros(store_rows * 40, np.uint16))
    # tracks: padded, shorter than `frames`, reaching the last row of the store, in the middle of it
    shapes = [(2, 3), (frames + 3, 40), (0, frames - 1), (5, 600), (0, 850), (1, 300), (7, 899), (0, 10), (3, 200)]
    starts = [0, 10, 20, 100, 50, 600, 1, 890, 400]
    win = np.array([(0, pad, rows, 0, 40 * at) for (pad, rows), at in zip(shapes, starts)], native.WINDOW_DTYPE)
    assert all(at + rows <= store_rows for (_, rows), at in zip(shapes, starts))
    probs = [(rng.integers(0, 9, n) / 8.0).astype(np.float32) for n in LENGTHS]
    probs[ALL_EQUAL][:] = np.float32(0.625)
    probs[NEG_ZERO][:] = np.float32(-0.0)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    st.set_probs(np.concatenate(probs))
    return st, win, off, probs, frames


def chain(probs, win, frames, stride, mode, window, cooldown, cutoff, before, after, max_new):
    """today's chain on the host: (clips, events, detections, per-track counts)"""
    mas = [streaming.moving_average_in_order(p, window) for p in probs]
    at = streaming.detection_positions(mas, cutoff, cooldown)
    ev = np.array([(t, int(i), mas[t][i]) for t in range(len(probs)) for i in at[t]], native.DETECTION_DTYPE).reshape(-1)
    counts = np.array([a.size for a in at], np.int64)
    total = ev.size
    if max_new is not None and ev.size > max_new:
        best = np.argsort(-ev["average"].astype(np.float64), kind="stable")[:max_new]
        ev = ev[np.sort(best)]
    clips, kept = streaming.detection_clips(win, ev, frames, stride, mode, window, before, after, return_kept=True)
    return clips, ev[kept], total, counts


def check_kernel(lib, stride, mode):
    st, win, off, probs, frames = kernel_case(lib, stride, mode)
    kind = np.zeros(win.size, np.int32)
    seen = dict(dropped=0, clipped=0, ties_cut=0, most=0)
    context = [(0, 0), (frames + 50, 1000)]   # exactly the window that fired; past both ends of the store
    cases = [(w, cd, cut, ctx) for w in (1, 5) for cd in (0, 1, 5, 25) for cut, ctx in ((0.25, context[(w + cd) % 2]), (-1.0, context[cd % 2]))]
    for window, cooldown, cutoff, (before, after) in cases:
        what = dict(stride=stride, mode=mode, window=window, cooldown=cooldown, cutoff=cutoff, before=before, after=after)
        _, d_count, _, _ = st.detections(off, kind, cutoff, window, 0, cooldown, capacity=0)
        K = int(d_count.sum())
        assert K > 20, what
        for max_new in (0, 1, K - 1, K, K + 1, None):
            what["max_new"] = max_new
            want_clips, want_ev, want_total, want_counts = chain(probs, win, frames, stride, mode, window, cooldown, cutoff, before, after, max_new)
            clips, ev, total, counts = st.mine(win, off, cutoff, window, cooldown, before, after, max_new)
            assert clips.tobytes() == want_clips.tobytes(), (what, clips[:4], want_clips[:4], clips.size, want_clips.size)
            assert dc.same_events(ev, want_ev), (what, ev[:4], want_ev[:4])
            assert total == want_total == K and np.array_equal(counts, want_counts) and np.array_equal(counts, d_count), what
            # a second call writes the same bytes
            clips2, ev2, total2, counts2 = st.mine(win, off, cutoff, window, cooldown, before, after, max_new)
            assert clips2.tobytes() == clips.tobytes() and ev2.tobytes() == ev.tobytes() and total2 == total and counts2.tobytes() == counts.tobytes(), what
            # what the case exercised, judged on the chain
            kept_n = K if max_new is None else min(max_new, K)
            seen["dropped"] += int(want_clips.size < kept_n)
            seen["clipped"] += int(np.any(want_clips["copy_rows"] < frames + before + after))
            seen["most"] = max(seen["most"], K)   # several workgroups of events
            if max_new is not None and 0 < max_new < K:
                avg = np.sort(chain(probs, win, frames, stride, mode, window, cooldown, cutoff, 0, 0, None)[1]["average"])[::-1]
                seen["ties_cut"] += int(max_new < avg.size and avg[max_new - 1] == avg[max_new])
        # a capacity below the result: the whole count, the exact prefix
        full, full_ev, _, _ = st.mine(win, off, cutoff, window, cooldown, before, after, K - 1)
        cap = full.size // 2
        some, some_ev, total, counts = st.mine(win, off, cutoff, window, cooldown, before, after, K - 1, capacity=cap)
        assert some.tobytes() == full[:cap].tobytes() and dc.same_events(some_ev, full_ev[:cap]) and total == K, what
    assert seen["dropped"] and seen["clipped"] and seen["ties_cut"] and seen["most"] > 2 * 1024, seen
    # -0.0 compares equal to +0.0: at cutoff -1 the all-(-0) track and the zeros elsewhere tie, the earlier event wins
    assert np.all(np.signbit(probs[NEG_ZERO])) and any(np.any(p == 0) and not np.any(np.signbit(p)) for p in probs[:NEG_ZERO] if p.size)
    # a cutoff nothing exceeds: no event, no clip
    clips, ev, total, counts = st.mine(win, off, 2.0, 5, 25)
    assert clips.size == 0 and ev.size == 0 and total == 0 and not counts.any()
    st.close()


def check_kernel_validation(lib):
    st, win, off, _, _ = kernel_case(lib, 1, "stream")
    for bad in (dict(off=off + 1), dict(off=off[::-1].copy()), dict(window=0), dict(cooldown=-1)):
        a = dict(dict(off=off, window=5, cooldown=2), **bad)
        with pytest.raises(native.NativeError, match="error"):
            st.mine(win, a["off"], 0.5, a["window"], a["cooldown"])
    with pytest.raises(ValueError, match="offsets"):
        st.mine(win, off[:-1], 0.5)
    st.close()


# ------------------------------------------------------------------------------------------------- through a model
def same_report(a, b):
    return set(a) == set(b) and all(a[k] == b[k] for k in a)


def check_through_model(lib, mode, quantized=False):
    """mine_hard_negatives_on_device == mine_hard_negatives on the handler of mining_checks.make_handler, clips and report"""
    model, fh = mc.make_handler(lib)
    if quantized:
        import q8_checks as qc
        _, qmodel, qm = qc.make_quantized(lib, ec.DEF, mc.T)
        fh = FeatureHandler(_handler_config(), engine=qmodel.engine)
        sm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=qmodel)
    else:
        sm = streaming.StreamingModel(model, 1, mode)
    cutoff = mc.median_cutoff(sm, fh)
    some = 0
    for kw in (dict(), dict(max_new=3), dict(max_new=3, before=10, after=6, ignore_slices_after_accept=5), dict(ignore_slices_after_accept=5, sliding_window_length=1)):
        st0 = mc.rng_state()
        want_clips, want = mining.mine_hard_negatives(sm, fh, cutoff, **kw)
        clips, report = mining.mine_hard_negatives_on_device(sm, fh, cutoff, **kw)
        assert clips.dtype == want_clips.dtype and clips.tobytes() == want_clips.tobytes(), (kw, clips, want_clips)
        assert same_report(report, want), (kw, report, want)
        assert mc.same_rng(mc.rng_state(), st0)
        some += clips.size
    assert some >= 10
    none, report = mining.mine_hard_negatives_on_device(sm, fh, 2.0)
    assert none.size == 0 and none.dtype == native.WINDOW_DTYPE and same_report(report, mining.mine_hard_negatives(sm, fh, 2.0)[1])


def _handler_config():
    from microwakeword_amd.synthetic import synthetic_stores
    pos, neg = synthetic_stores(10, 77, min_len=60, max_len=220)
    _, neg_f = synthetic_stores(6, 78, dtype=np.float32, min_len=mc.T - 8, max_len=150)
    return {"stride": 1, "window_step_ms": 20, "features": [
        dict(type="mmap", stores={"training": [pos]}, truth=True, sampling_weight=2.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
        dict(type="mmap", stores={"training": [neg]}, truth=False, sampling_weight=5.0, penalty_weight=1.5, truncation_strategy="random"),
        dict(type="mmap", stores={"training": [neg_f]}, truth=False, sampling_weight=3.0, penalty_weight=0.5, truncation_strategy="truncate_end")]}


# ------------------------------------------------------------------------------------------------- set_mined_clips
def check_set_mined_clips_refusals(lib):
    model, fh = mc.make_handler(lib)
    sid = fh.feature_providers[1].store_id["u16"]
    size = fh.feature_providers[1].flat["u16"].size
    ok = (sid, 0, 60, 0, 0)
    mined = fh.add_mined_provider(np.array([ok], native.WINDOW_DTYPE), sampling_weight=0.5, penalty_weight=0.25)
    for bad in [(sid, 0, 60, 0, size - 59 * 40), (sid, 0, 60, 0, 7), (sid, 0, 0, 0, 0), (sid, 0, 60, 0, -40), (17, 0, 60, 0, 0), (sid, 2, 60, 0, 0)]:
        with pytest.raises(ValueError, match="clip 1"):
            fh.set_mined_clips(mined, np.array([ok, bad], native.WINDOW_DTYPE))
    with pytest.raises(ValueError, match="no clips"):
        fh.set_mined_clips(mined, np.zeros(0, native.WINDOW_DTYPE))
    assert mined.samples == [(0, 0, 60)] and len(fh.feature_providers) == 4   # a refused call changes nothing
    with pytest.raises(ValueError, match="mined provider"):
        fh.set_mined_clips(fh.feature_providers[1], np.array([ok], native.WINDOW_DTYPE))
    _, other = mc.make_handler(lib)
    with pytest.raises(ValueError, match="mined provider"):
        other.set_mined_clips(mined, np.array([ok], native.WINDOW_DTYPE))
    # the replacement: no upload, no draw, the provider's place, weights and sizes
    uploaded, st0 = fh.uploaded_bytes, mc.rng_state()
    new = np.array([(sid, 0, 70, 0, 40 * 3), (sid, 0, 52, 0, size - 52 * 40), ok], native.WINDOW_DTYPE)
    assert fh.set_mined_clips(mined, new) is mined and fh.feature_providers[-1] is mined
    assert fh.uploaded_bytes == uploaded and mc.same_rng(mc.rng_state(), st0)
    assert mined.get_mode_size("training") == 3 and mined.sampling_weight == 0.5 and mined.penalty_weight == 0.25 and mined.label == 0.0
    # only the mined provider drawn: every window is a new clip's truncate_start window
    for p in fh.feature_providers[:-1]:
        p.sampling_weight = 0.0
    fh._sampler = None
    b = fh.draw_training_batch(mc.B, mc.T, "default", None)
    drawn = b["sample"][b["order"]]
    assert set(drawn.tolist()) == {0, 1, 2}
    for j in range(mc.B):
        assert tuple(b["windows"][j].tolist()) == mc.expected_window(new[drawn[j]], mc.T), j


def check_set_mined_clips_weight_zero(lib):
    """a running prefetcher: replacing the clips of a weight-0 provider between two batches leaves the batches that follow as
    they were (what mining_checks.check_prefetcher_is_rebuilt pins for add_mined_provider)"""
    out = []
    for replace in (False, True):
        model, fh = mc.make_handler(lib)
        src = fh.feature_providers[1]
        mined = fh.add_mined_provider(np.array([(src.store_id["u16"], 0, 70, 0, 40 * 3)], native.WINDOW_DTYPE), sampling_weight=0.0)
        fh.use_private_rng(prefetch=2)
        fh.next_training_batch_on_device(mc.B, mc.T, augmentation_policy=ec.POLICY)
        if replace:
            st0 = mc.rng_state()
            fh.set_mined_clips(mined, np.array([(src.store_id["u16"], 0, 55, 0, 40 * 9), (src.store_id["u16"], 0, 61, 0, 0)], native.WINDOW_DTYPE))
            assert mc.same_rng(mc.rng_state(), st0) and mined.get_mode_size("training") == 2
        got = []
        for _ in range(2):
            y, w = fh.next_training_batch_on_device(mc.B, mc.T, augmentation_policy=ec.POLICY, want_targets=True)
            got.append((model.engine.get_batch(mc.B).tobytes(), np.asarray(y).tobytes(), np.asarray(w).tobytes()))
        out.append(got)
        fh.release_private_rng()
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------------- the loop
T_LOOP, B_LOOP, STEPS = 60, 16, 12
MINING = dict(cutoff=0.0, ignore_slices_after_accept=5, max_new=7)


def loop_config(tmp_path, name, mining_map=None):
    cfg = dict(ec.learnable_config(T=T_LOOP), train_dir=str(tmp_path / name), summaries_dir=str(tmp_path / name / "logs"), batch_size=B_LOOP,
               spectrogram_length=T_LOOP, training_steps=[STEPS // 2, STEPS - STEPS // 2], learning_rates=[0.01, 0.003],
               time_mask_max_size=[0], time_mask_count=[0], freq_mask_max_size=[0], freq_mask_count=[0],
               positive_class_weight=[1.0], negative_class_weight=[1.0], eval_step_interval=STEPS // 3, target_minimization=0.9,
               minimization_metric=None, maximization_metric="accuracy")
    if mining_map is not None:
        cfg["hard_negative_mining"] = dict(mining_map)
    return cfg


def run_loop(lib, cfg, steps=None):
    """the run of engine_checks.check_train_loop_end_to_end: the same seeds every time -> (model, handler)"""
    from microwakeword_amd import mixednet
    from microwakeword_amd import train as tr
    random.seed(1)
    np.random.seed(1)
    model = mixednet.model(ec.DEF, (T_LOOP, 40), B_LOOP, lib=lib, seed=7, max_batch=64)
    fh = FeatureHandler(cfg, engine=model.engine)
    tr.train(model, cfg, fh, verbose=False)
    return model, fh


def mined_file(cfg):
    with np.load(os.path.join(cfg["train_dir"], "mined_clips.npz")) as z:
        return {k: z[k] for k in ("provider", "dtype_key", "src_elem", "rows", "round")}


def mining_log(cfg):
    with open(os.path.join(cfg["summaries_dir"], "mining", "scalars.jsonl")) as fh:
        return [json.loads(line) for line in fh]


def rows_of(clips, fh):
    """clips as (provider index, dtype key, src_elem, rows), the columns of mined_clips.npz"""
    where = {int(sid): (i, key) for i, p in enumerate(fh.feature_providers) if getattr(p, "flat", None) for key, sid in p.store_id.items()}
    return [(where[int(c["store"])][0], where[int(c["store"])][1], int(c["src_elem"]), int(c["copy_rows"])) for c in clips]


def file_rows(z, rnd=None):
    pick = np.arange(z["round"].size) if rnd is None else np.nonzero(z["round"] == rnd)[0]
    return [(int(z["provider"][j]), str(z["dtype_key"][j]), int(z["src_elem"][j]), int(z["rows"][j])) for j in pick]


def by_hand_round_one(lib, cfg):
    """mine_hard_negatives by hand on a fresh model loaded with the weights file the run of `cfg` saved at step 4"""
    from microwakeword_amd import mixednet
    first = [f for f in os.listdir(os.path.join(cfg["train_dir"], "train")) if "_weights_4." in f]
    assert len(first) == 1
    random.seed(1)
    np.random.seed(1)
    fresh = mixednet.model(ec.DEF, (T_LOOP, 40), B_LOOP, lib=lib, seed=99, max_batch=64)
    fresh.load_weights(os.path.join(cfg["train_dir"], "train", first[0].replace(".npz", "")))
    fh = FeatureHandler(cfg, engine=fresh.engine)
    sm = streaming.StreamingModel(fresh, int(cfg["stride"]), "stream")
    by_hand, rep = mining.mine_hard_negatives(sm, fh, 0.0, max_new=7, ignore_slices_after_accept=5)
    return by_hand, rep, fh


def check_loop_rounds(lib, tmp_path):
    """runs A (no key), B (mining at every boundary), B' (B at sampling weight 0)"""
    cfg_a = loop_config(tmp_path, "a")
    model_a, _ = run_loop(lib, cfg_a)
    last_a = [w.copy() for w in model_a.get_weights()]
    assert not os.path.exists(os.path.join(cfg_a["train_dir"], "mined_clips.npz")) and not os.path.isdir(os.path.join(cfg_a["summaries_dir"], "mining"))
    # B: rounds at steps 4 and 8 only, two log lines
    cfg_b = loop_config(tmp_path, "b", MINING)
    model_b, fh_b = run_loop(lib, cfg_b)
    log = mining_log(cfg_b)
    assert [int(e["step"]) for e in log] == [4, 8], log
    assert all(set(e) == {"step", "detections", "kept", "total", "hours", "detections_per_hour"} for e in log)
    assert all(e["detections"] > 0 and 0 < e["kept"] <= 7 and e["hours"] > 0 for e in log)
    assert all(e["detections_per_hour"] == e["detections"] / e["hours"] for e in log)
    z = mined_file(cfg_b)
    assert set(z["round"].tolist()) <= {1, 2} and log[1]["total"] == z["round"].size <= 14
    mined = fh_b.feature_providers[-1]
    assert mined.get_mode_size("training") == z["round"].size and mined.sampling_weight == 1.0 and mined.label == 0.0
    # round 1 is what mine_hard_negatives returns by hand on a fresh model with A's step-4 weights.  Up to step 4 the runs A
    # and B are the same run, and A saved its step-4 weights at that boundary (train/<best>_weights_4.weights.h5)
    by_hand, rep, fh = by_hand_round_one(lib, cfg_a)
    assert log[0]["detections"] == rep["detections"] and log[0]["kept"] == rep["count"] == by_hand.size
    # A round-1 clip that round 2 mined again moved to the end and carries round 2: B's round-1 rows are the by-hand clips that
    # round 2 did not mine again, in their order (check_loop_merge_and_restore holds a run cut after its first round to all of them)
    again = set(file_rows(z, 2))
    assert file_rows(z, 1) == [r for r in rows_of(by_hand, fh) if r not in again], (file_rows(z), rows_of(by_hand, fh))
    # which boundaries are due: every n-th, not before first_step, never the last step
    class _Rounds(mining.MiningRounds):   # noqa: E306
        def __init__(self, **kw):
            self.m, self.boundaries = mining.mining_config(dict(hard_negative_mining=dict(MINING, **kw))), 0
    r = _Rounds(every_evals=2, first_step=5)
    assert [st for st in (2, 4, 6, 8, 10, 12) if r.due(st, st == 12)] == [8]
    r = _Rounds()
    assert [st for st in (4, 8, 12) if r.due(st, st == 12)] == [4, 8]
    # B': sampling weight 0 -> A's weights, bit for bit
    cfg_z = loop_config(tmp_path, "z", dict(MINING, sampling_weight=0.0))
    model_z, fh_z = run_loop(lib, cfg_z)
    assert len(mining_log(cfg_z)) == 2 and fh_z.feature_providers[-1].get_mode_size("training") > 0
    for a, b in zip(last_a, model_z.get_weights()):
        assert a.tobytes() == b.tobytes()
    la = np.load(os.path.join(cfg_a["train_dir"], "last_weights.weights.h5.npz"))
    lz = np.load(os.path.join(cfg_z["train_dir"], "last_weights.weights.h5.npz"))
    assert sorted(la.files) == sorted(lz.files) and all(la[k].tobytes() == lz[k].tobytes() for k in la.files)
    # and with weight 1 the mined clips are drawn: the run differs from A
    assert any(a.tobytes() != b.tobytes() for a, b in zip(last_a, model_b.get_weights()))


def check_loop_no_detections(lib, tmp_path):
    cfg = loop_config(tmp_path, "none", dict(MINING, cutoff=1.0))
    _, fh = run_loop(lib, cfg)
    log = mining_log(cfg)
    assert [int(e["step"]) for e in log] == [4, 8] and all(e["detections"] == 0 and e["kept"] == 0 and e["total"] == 0 for e in log)
    assert len(fh.feature_providers) == len(cfg["features"]) and not os.path.exists(os.path.join(cfg["train_dir"], "mined_clips.npz"))


def check_loop_merge_and_restore(lib, tmp_path):
    """max_total 10 with max_new 7: the list after round 2 as the merge rule orders it; a restored run picks it up"""
    cfg1 = loop_config(tmp_path, "one", MINING)
    cfg1["training_steps"] = [6, 2]   # one round, at step 4
    run_loop(lib, cfg1)
    z1 = mined_file(cfg1)
    assert [int(e["step"]) for e in mining_log(cfg1)] == [4]   # 8 steps: the boundary at 8 is the last step
    by_hand, _, fh1 = by_hand_round_one(lib, cfg1)
    assert set(z1["round"].tolist()) == {1} and file_rows(z1) == rows_of(by_hand, fh1), (file_rows(z1), rows_of(by_hand, fh1))
    cfg = loop_config(tmp_path, "two", dict(MINING, max_total=10))
    _, fh = run_loop(lib, cfg)
    z = mined_file(cfg)
    log = mining_log(cfg)
    r1, rows = file_rows(z1), file_rows(z)
    second = file_rows(z, 2)
    assert len(rows) <= 10 and log[1]["total"] == len(rows) and len(second) == log[1]["kept"] > 0
    assert rows[len(rows) - len(second):] == second and z["round"].tolist() == sorted(z["round"].tolist())
    # round 1's clips that round 2 did not mine again, in their order, dropped from the front beyond max_total
    survivors = [r for r in r1 if r not in set(second)]
    assert rows[:len(rows) - len(second)] == survivors[max(len(survivors) + len(second) - 10, 0):]
    # the merge rule itself, on a list where every branch is taken
    w = lambda *keys: np.array([(0, 0, r, 0, e) for e, r in keys], native.WINDOW_DTYPE).reshape(-1)   # noqa: E731
    clips, rounds = mining.merge_clips(w((0, 5), (40, 5), (80, 5), (120, 5)), [1, 1, 2, 2], w((80, 5), (40, 6), (80, 5), (0, 5)), 3, 5)
    assert [(int(c["src_elem"]), int(c["copy_rows"])) for c in clips] == [(40, 5), (120, 5), (80, 5), (40, 6), (0, 5)] and rounds.tolist() == [1, 2, 3, 3, 3]
    # a restored run (the checkpoint is in train_dir) starts with the list and merges into it
    cfg_r = dict(cfg, training_steps=[6, 2])
    model_r, fh_r = run_loop(lib, cfg_r)
    assert fh_r.feature_providers[-1].get_mode_size("training") > 0
    zr = mined_file(cfg_r)
    assert set(zr["round"].tolist()) <= {1, 2, 3} and 3 in zr["round"].tolist() and zr["round"].size <= 10
    third = file_rows(zr, 3)
    kept_old = [r for r in rows if r not in set(third)]
    assert file_rows(zr)[:len(file_rows(zr)) - len(third)] == kept_old[max(len(kept_old) + len(third) - 10, 0):]
    # a list that no longer fits its stores: a warning, an empty start
    np.savez(os.path.join(cfg_r["train_dir"], "mined_clips.npz"), provider=z["provider"], dtype_key=z["dtype_key"],
             src_elem=z["src_elem"] + 10 ** 9, rows=z["rows"], round=z["round"])
    from microwakeword_amd import mixednet
    model = mixednet.model(ec.DEF, (T_LOOP, 40), B_LOOP, lib=lib, seed=7, max_batch=64)
    fh = FeatureHandler(cfg_r, engine=model.engine)
    rounds = mining.MiningRounds(mining.mining_config(cfg_r), model, fh, cfg_r, writer=None)
    assert rounds.path is None   # no writer: not the chief, no file
    class _W:   # noqa: E306
        def scalars(self, step, **kv):
            pass
    rounds = mining.MiningRounds(mining.mining_config(cfg_r), model, fh, cfg_r, writer=_W())
    assert rounds.clips.size == 0 and rounds.provider is None and len(fh.feature_providers) == len(cfg_r["features"])


def check_loop_refusals(lib, tmp_path, monkeypatch):
    from microwakeword_amd import mixednet, model_train_eval
    from microwakeword_amd import train as tr
    for bad, word in ((dict(MINING, every=2), "every"), (dict(max_new=3), "cutoff"), (dict(MINING, every_evals=0), "every_evals"),
                      (dict(MINING, max_total=3), "max_total"), (dict(MINING, mode="both"), "mode"), (dict(MINING, before=-1), "before"),
                      (dict(MINING, max_new="many"), "integers")):
        with pytest.raises(ValueError, match="hard_negative_mining.*" + word):
            mining.mining_config(dict(hard_negative_mining=bad))
    assert mining.mining_config({}) is None
    full = mining.mining_config(dict(hard_negative_mining=dict(cutoff=0.5)))
    assert full == dict(cutoff=0.5, every_evals=1, first_step=0, max_new=2000, max_total=10000, sampling_weight=1.0, penalty_weight=1.0, mode="stream",
                        sliding_window_length=5, ignore_slices_after_accept=25, before=0, after=0)
    # a handler and a model on two engines
    cfg = loop_config(tmp_path, "two_engines", MINING)
    model = mixednet.model(ec.DEF, (T_LOOP, 40), B_LOOP, lib=lib, seed=7, max_batch=64)
    other = mixednet.model(ec.DEF, (T_LOOP, 40), B_LOOP, lib=lib, seed=7, max_batch=64)
    with pytest.raises(ValueError, match="hard_negative_mining.*one engine"):
        tr.train(model, cfg, FeatureHandler(cfg, engine=other.engine), verbose=False)
    # a world of 2: before the first step
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    cfg = loop_config(tmp_path, "world", MINING)
    fh = FeatureHandler(cfg, engine=model.engine)
    with pytest.raises(ValueError, match="hard_negative_mining.*world size 2"):
        tr.train(model, cfg, fh, verbose=False)
    assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    # the command line: before train_dir is claimed (and before a model is built)
    import yaml
    train_dir = tmp_path / "cli_run"
    with open(tmp_path / "training_parameters.yaml", "w") as out:
        yaml.safe_dump(dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=B_LOOP, features=[], hard_negative_mining=dict(MINING)), out)
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet"]
    with pytest.raises(ValueError, match="hard_negative_mining.*world size 2"):
        model_train_eval.main(argv)
    assert not train_dir.exists()
    with open(tmp_path / "training_parameters.yaml", "w") as out:
        yaml.safe_dump(dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=B_LOOP, features=[], hard_negative_mining=dict(MINING, evry=1)), out)
    with pytest.raises(ValueError, match="hard_negative_mining.*evry"):
        model_train_eval.main(argv)
    assert not train_dir.exists()
