"""Checks of hard-negative mining (microwakeword_amd/mining.py, FeatureHandler.add_mined_provider) shared by the emulator
tests (tests/test_mining_emulated.py) and the GPU tests (tests/test_mining_gpu.py)."""
import logging
import random

import numpy as np
import pytest

from microwakeword_amd import mining, native, streaming
from microwakeword_amd.data import FeatureHandler
from microwakeword_amd.synthetic import synthetic_stores
import engine_checks as ec
import streaming_checks as sc

T = 52
B = 24


def make_handler(lib, shard=None, seed=5):
    _, model = sc.make_model(lib, ec.DEF, T)
    pos, neg = synthetic_stores(10, 77, min_len=60, max_len=220)
    _, neg_f = synthetic_stores(6, 78, dtype=np.float32, min_len=T - 8, max_len=150)
    cfg = {"stride": 1, "window_step_ms": 20, "features": [
        dict(type="mmap", stores={"training": [pos], "testing": [pos[:2]]}, truth=True, sampling_weight=2.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
        dict(type="mmap", stores={"training": [neg], "testing": [neg[:3]]}, truth=False, sampling_weight=5.0, penalty_weight=1.5, truncation_strategy="random"),
        dict(type="mmap", stores={"training": [neg_f]}, truth=False, sampling_weight=3.0, penalty_weight=0.5, truncation_strategy="truncate_end")]}
    random.seed(seed)
    np.random.seed(seed)
    return model, FeatureHandler(cfg, engine=model.engine, shard=shard)


def rng_state():
    return random.getstate(), np.random.get_state()


def same_rng(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def set_rng(st):
    random.setstate(st[0])
    np.random.set_state(st[1])


def restated_events(sm, fh, mode, cutoff, w=5, cooldown=25):
    """the detections of the label-0 tracks of `mode` from the probabilities read back, by the NumPy restatement"""
    win, _ = fh.track_windows(mode, sm.frames, only_label=0.0)
    sm.reset()
    off = sm.native.run(win)
    p = sm.read_probabilities()
    mas = [streaming.moving_average_in_order(p[off[t]:off[t + 1]], w) for t in range(win.size)]
    at = streaming.detection_positions(mas, cutoff, cooldown)
    ev = [(t, int(i), mas[t][i]) for t in range(win.size) for i in at[t]]
    return win, np.array(ev, native.DETECTION_DTYPE).reshape(-1), mas


def median_cutoff(sm, fh, mode="training"):
    _, _, mas = restated_events(sm, fh, mode, 2.0)
    return float(np.median(np.concatenate(mas)))


def expected_window(clip, T):
    """the truncate_start window of a clip: its last T rows (a shorter clip whole, left-padded)"""
    rows, elem = int(clip["copy_rows"]), int(clip["src_elem"])
    if rows > T:
        return (int(clip["store"]), 0, T, 0, elem + (rows - T) * 40)
    return (int(clip["store"]), T - rows, rows, 0, elem)


def host_window(mined, i, T):
    x = mined.host_rows(i)[-T:]
    return np.concatenate([np.zeros((T - x.shape[0], 40), np.float32), x], 0)


def check_mining_and_mined_provider(lib, mode="non_stream"):
    model, fh = make_handler(lib)
    sm = streaming.StreamingModel(model, 1, mode)
    cutoff = median_cutoff(sm, fh)
    win, want_ev, mas = restated_events(sm, fh, "training", cutoff, cooldown=5)
    clips, report = mining.mine_hard_negatives(sm, fh, cutoff, before=10, after=6, ignore_slices_after_accept=5)
    want_clips = streaming.detection_clips(win, want_ev, T, 1, mode, 5, before=10, after=6)
    assert clips.size >= 10 and clips.tobytes() == want_clips.tobytes()
    assert report["count"] == clips.size and report["detections"] == want_ev.size and report["tracks"] == win.size == 16
    assert sum(report["per_provider"].values()) == clips.size and set(report["per_provider"]) <= {1, 2}
    assert report["hours"] == streaming.track_hours([m.size for m in mas], 1, 0.02)
    assert np.any(clips["copy_rows"] > T) and np.any(clips["copy_rows"] < T + 16)   # truncated by the sampler / clipped by the store
    # max_new: the highest averages, ties to the earlier event, returned in (track, index) order
    few, rep = mining.mine_hard_negatives(sm, fh, cutoff, max_new=3, ignore_slices_after_accept=5)
    top = sorted(sorted(range(want_ev.size), key=lambda j: (-float(want_ev["average"][j]), j))[:3])
    assert few.tobytes() == streaming.detection_clips(win, want_ev[top], T, 1, mode, 5).tobytes() and rep["detections"] == want_ev.size

    # ---- the provider: no upload, no RNG draw, sizes
    sizes = {m: fh.get_mode_size(m) for m in ("training", "testing", "validation")}
    durations = {m: fh.get_mode_duration(m) for m in ("training", "testing", "validation")}
    before_draw = rng_state()
    b_without = fh.draw_training_batch(B, T, "default", ec.POLICY)
    set_rng(before_draw)
    uploaded, st0 = fh.uploaded_bytes, rng_state()
    mined = fh.add_mined_provider(clips, sampling_weight=0.0, penalty_weight=0.75)
    assert fh.uploaded_bytes == uploaded and same_rng(rng_state(), st0)
    assert fh.get_mode_size("training") == sizes["training"] + clips.size
    assert fh.get_mode_duration("training") == durations["training"] + sum(0.02 * int(r) for r in clips["copy_rows"])
    assert all(fh.get_mode_size(m) == sizes[m] and fh.get_mode_duration(m) == durations[m] for m in ("testing", "validation"))
    assert all(mined.get_mode_size(m) == 0 and mined.get_mode_duration(m) == 0 for m in ("testing", "validation", "testing_ambient"))
    # at sampling weight 0 the batches are the ones drawn without it, bit for bit
    b_with = fh.draw_training_batch(B, T, "default", ec.POLICY)
    for k in ("windows", "masks", "labels", "weights", "order", "provider", "sample"):
        assert np.asarray(b_with[k]).tobytes() == np.asarray(b_without[k]).tobytes(), k

    # ---- only the mined provider drawn: every window is a clip's truncate_start window
    for p in fh.feature_providers[:-1]:
        p.sampling_weight = 0.0
    mined.sampling_weight = 1.0
    fh._sampler = None
    st = rng_state()
    b = fh.draw_training_batch(B, T, "default", None)
    assert np.all(b["provider"] == len(fh.feature_providers) - 1) and len(set(b["sample"].tolist())) > 3
    drawn = b["sample"][b["order"]]
    for j in range(B):
        assert tuple(b["windows"][j].tolist()) == expected_window(clips[drawn[j]], T), j
    assert np.all(b["labels"] == 0.0) and np.all(b["weights"] == 0.75)
    set_rng(st)
    x, y, w = fh.get_data("training", B, T, "default", None)
    assert np.all(y == 0.0) and np.all(w == 0.75)
    for j in range(B):
        assert np.array_equal(x[j], host_window(mined, int(drawn[j]), T)), j
    # the device path serves them too
    y, w = fh.next_training_batch_on_device(B, T)
    served = model.engine.get_batch(B)
    known = {host_window(mined, i, T).tobytes() for i in range(clips.size)}
    assert np.all(np.asarray(y) == 0.0) and all(served[j].tobytes() in known for j in range(B))
    # with before = after = 0 the truncate_start window is exactly the window that fired
    exact = streaming.detection_clips(win, want_ev, T, 1, mode, 5)
    full = exact[exact["copy_rows"] == T]
    assert full.size and all(expected_window(c, T) == tuple(c.tolist()) for c in full)


def check_prefetcher_is_rebuilt(lib):
    """a running prefetcher: adding a provider at weight 0 between two batches leaves the batches that follow as they were"""
    out = []
    for add in (False, True):
        model, fh = make_handler(lib)
        fh.use_private_rng(prefetch=2)
        fh.next_training_batch_on_device(B, T, augmentation_policy=ec.POLICY)
        if add:
            src = fh.feature_providers[1]
            clip = np.array([(src.store_id["u16"], 0, 70, 0, 40 * 3)], native.WINDOW_DTYPE)
            fh.add_mined_provider(clip, sampling_weight=0.0)
        got = []
        for _ in range(2):
            y, w = fh.next_training_batch_on_device(B, T, augmentation_policy=ec.POLICY, want_targets=True)
            got.append((model.engine.get_batch(B).tobytes(), np.asarray(y).tobytes(), np.asarray(w).tobytes()))
        out.append(got)
        fh.release_private_rng()
    assert out[0] == out[1]


def check_refusals(lib):
    model, fh = make_handler(lib)
    sid = fh.feature_providers[1].store_id["u16"]
    size = fh.feature_providers[1].flat["u16"].size
    ok = (sid, 0, 60, 0, 0)
    for bad in [(sid, 0, 60, 0, size - 59 * 40), (sid, 0, 60, 0, 7), (sid, 0, 0, 0, 0), (sid, 0, 60, 0, -40), (17, 0, 60, 0, 0), (sid, 2, 60, 0, 0)]:
        with pytest.raises(ValueError, match="clip 1"):
            fh.add_mined_provider(np.array([ok, bad], native.WINDOW_DTYPE))
    assert len(fh.feature_providers) == 3
    fh.add_mined_provider(np.array([ok, (sid, 0, 60, 0, size - 60 * 40)], native.WINDOW_DTYPE))   # the last rows of the store
    with pytest.raises(NotImplementedError, match="shard"):
        fh.shard_training_lists(0, 2)
    _, sharded = make_handler(lib, shard=(0, 2))
    with pytest.raises(NotImplementedError, match="shard of the training rows"):
        sharded.add_mined_provider(np.array([ok], native.WINDOW_DTYPE))


def check_testing_mode_warns(lib, caplog):
    model, fh = make_handler(lib)
    sm = streaming.StreamingModel(model, 1, "stream")
    with caplog.at_level(logging.WARNING):
        clips, report = mining.mine_hard_negatives(sm, fh, median_cutoff(sm, fh, "testing"), mode="testing")
    assert "contaminates" in caplog.text and report["mode"] == "testing" and report["tracks"] == 3
    win, want_ev, _ = restated_events(sm, fh, "testing", report["cutoff"])
    assert clips.tobytes() == streaming.detection_clips(win, want_ev, T, 1, "stream", 5).tobytes()
