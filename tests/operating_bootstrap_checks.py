"""Checks of mww_stream_operating_bootstrap (csrc/tu_stream_bootstrap.hip through microwakeword_amd.streaming) shared by the
emulator tests (tests/test_operating_bootstrap_emulated.py) and the GPU tests (tests/test_operating_bootstrap_gpu.py): the same
shapes on both.  Every assertion on the device's records is byte equality against the NumPy restatement
(``streaming.bootstrap_units_host`` + ``bootstrap_records_host`` = ``operating_bootstrap_host``), and two calls must write the
same bytes; there is no tolerance.  The generators and cases of tests/operating_point_checks.py and
tests/operating_summary_checks.py are used as they are."""
import numpy as np
import pytest

from microwakeword_amd import native, streaming
import engine_checks as ec
import operating_point_checks as oc
import operating_summary_checks as osc
import stream_detect_checks as dc
import streaming_checks as sc

S = oc.S                 # POST_SEG = MWW_BOOT_BLOCK_UNIT
P = 256                  # threads of boot_level_kernel and of boot_replicate_kernel (BOOT_THREADS of csrc/tu_stream_bootstrap.hip)
STRIDE, STEP = osc.STRIDE, osc.STEP
REPLICATES = (1, 63, 64, 65, P - 1, P, P + 1)   # around a wave and around the replicate kernel's workgroup
same = osc.same
assert S == native.BOOT_BLOCK_UNIT


# ---- draws
def draw_bigint(seed, kind, r, i, n):
    """the draw of include/mww.h in Python integers"""
    m = (1 << 64) - 1
    z = (seed + ((kind << 56) | (r << 32) | i) * 0x9E3779B97F4A7C15) & m
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & m
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & m
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def check_draws():
    idx = np.array([0, 1, 2, 63, 64, 1000, 2 ** 31 - 2, 2 ** 32 - 1], np.int64)
    for seed in (0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF):   # 2^64 - 1: the sum wraps
        for n in (1, 2, 101, 2 ** 31 - 1):
            for r in (0, 1, 65535):
                for kind in (0, 1):
                    got = streaming.bootstrap_draw(seed, kind, r, idx, n)
                    assert got.dtype == np.int64 and [int(v) for v in got] == [draw_bigint(seed, kind, r, int(i), n) for i in idx]
                    assert streaming.bootstrap_draw(seed, kind, r, 5, n) == draw_bigint(seed, kind, r, 5, n)
                    assert got.min() >= 0 and got.max() < n
    many = np.arange(4096)
    rows = {(k, r): streaming.bootstrap_draw(7, k, r, many, 1000).tobytes() for k in (0, 1) for r in (0, 1, 2, 65535)}
    assert len(set(rows.values())) == len(rows)   # draws of different (kind, r) differ
    d = streaming.bootstrap_draw(7, 0, 3, np.arange(100000), 10)
    assert np.bincount(d, minlength=10).min() > 9500   # every unit is drawn about as often


# ---- the device against the restatement
def usable_on_full_data(lengths, kind, windows, skip):
    kind = np.asarray(kind)
    left = np.asarray(lengths, np.int64) - np.where(kind != 0, skip, 0)
    return np.array([bool(np.any(kind == 0) and np.any(kind != 0) and np.all(left >= w)) for w in windows])


def split(tracks, kind):
    kind = np.asarray(kind)
    return [tracks[t] for t in np.nonzero(kind == 0)[0]], [tracks[t] for t in np.nonzero(kind != 0)[0]]


def check_records(st, tracks, off, kind, windows, cutoffs, skip, cooldown, block, replicates, seed, target, fixed, stride=STRIDE,
                  step_s=STEP, units=None):
    """mww_stream_operating_bootstrap == the restatement for every count of ``replicates`` (a replicate does not depend on how
    many there are: the restatement runs once, at the largest count), twice the same bytes; returns the restatement's records
    and units (``units``: those of the restatement on these tracks, when the caller has them)"""
    if units is None:
        units = streaming.bootstrap_units_host(*split(tracks, kind), windows, cutoffs, cooldown, block, skip)
    usable = usable_on_full_data([len(t) for t in tracks], kind, windows, skip)
    want = streaming.bootstrap_records_host(units, usable, np.asarray(windows, np.int64), cutoffs, stride, step_s, target, max(replicates), seed, fixed)
    for n in replicates:
        got = st.operating_bootstrap(off, kind, windows, cutoffs, skip, cooldown, stride, step_s, target, n, seed, block, fixed)
        assert got.dtype == native.BOOT_RECORD_DTYPE and same(got, want[:n]), (n, block, got[:4], want[:4])
    again = st.operating_bootstrap(off, kind, windows, cutoffs, skip, cooldown, stride, step_s, target, max(replicates), seed, block, fixed)
    assert again.tobytes() == want.tobytes()
    return want, units


def check_surface(sm, tracks, off, kind, windows, cutoffs, ignore, target, replicates, seed, block, confidence=0.9, fixed=None, stride=STRIDE,
                  step_s=STEP):
    """StreamingModel.operating_bootstrap == operating_bootstrap_host, key for key and byte for byte"""
    amb, pos = split(tracks, kind)
    want = streaming.operating_bootstrap_host(amb, pos, windows, cutoffs, stride, step_s, ignore, target, replicates, seed, block, confidence, fixed)
    got = sm.operating_bootstrap(off, kind, windows, cutoffs, ignore, stride, step_s, target, replicates, seed, block, confidence, fixed)
    assert set(got) == set(streaming.SUMMARY_KEYS) | set(streaming.SELECTION_KEYS) | {"bootstrap"}
    gb, wb = got.pop("bootstrap"), dict(want.pop("bootstrap"))
    osc.same_dict(got, want)
    assert set(gb) == set(wb) == {"records", "replicates", "seed", "block", "confidence", "fixed_row", "fixed_cutoff", "intervals"}
    assert same(gb["records"], wb["records"]), (gb["records"][:4], wb["records"][:4])
    assert gb["intervals"] == wb["intervals"] and all(gb[k] == wb[k] for k in wb if k not in ("records", "intervals"))
    for lo_hi in gb["intervals"].values():
        assert lo_hi is None or lo_hi[0] <= lo_hi[1]
    got["bootstrap"] = gb
    return got


def check_grid_cases(sm, case):
    """the inputs and cases of the operating-point tests - kinds interleaved, skip != cooldown, the repeated window - at block
    0 and S: first every track (lengths 0 and 4 are in the set: no window is usable, every record carries the fixed point
    alone), then the tracks that leave windows 1 .. 10 usable, re-selected at a target inside the grid's own FAPH range.
    The restatement's units are computed once, at block S on every track: a unit depends on its own track alone, and a
    non-empty track as one block is the sum of its blocks (check_block_borders compares that with the restatement at block 0)."""
    cooldown, skip, parity, cutoffs = oc.CASES[case]
    inp = oc.inputs()
    fixed = (2, len(cutoffs) // 3)
    all_kind = np.array([(t + parity) % 2 for t in range(len(inp.lengths))], np.int32)
    amb_ids, pos_ids = np.nonzero(all_kind == 0)[0], np.nonzero(all_kind == 1)[0]
    cnt, length, score = streaming.bootstrap_units_host(*split(inp.tracks, all_kind), oc.WINDOWS, cutoffs, cooldown, S, skip)
    first = np.concatenate([[0], np.cumsum([-(-inp.lengths[t] // S) for t in amb_ids])])
    for keep_short in (True, False):
        keep = lambda t: keep_short or inp.lengths[t] >= 40   # noqa: E731
        ids = [t for t in range(len(inp.lengths)) if keep(t)]
        tracks = [inp.tracks[t] for t in ids]
        off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
        kind = all_kind[ids]
        sm.native.set_probs(np.concatenate(tracks))
        rows = [np.arange(first[j], first[j + 1]) for j, t in enumerate(amb_ids) if keep(t)]
        pos = [i for i, t in enumerate(pos_ids) if keep(t)]
        units = {S: (cnt[:, np.concatenate(rows)], length[:, np.concatenate(rows)], score[:, pos]),
                 0: (np.stack([cnt[:, r].sum(axis=1, dtype=np.uint32) for r in rows], axis=1),
                     np.stack([length[:, r].sum(axis=1) for r in rows], axis=1), score[:, pos])}
        g = sm.operating_summary(off, kind, oc.WINDOWS, cutoffs, cooldown, STRIDE, STEP)
        usable = usable_on_full_data([len(t) for t in tracks], kind, oc.WINDOWS, skip)
        assert usable.any() != keep_short and (keep_short or list(usable) == [True] * 4 + [False, True])   # 256 is longer than most tracks
        # a target inside the FAPH range of window 5: some replicates meet it at a smaller cutoff than others
        target = 1.0 if keep_short else float(np.median(g["counts"][2].astype(np.float64) / g["hours"][2]))
        for block in (0, S):
            want, _ = check_records(sm.native, tracks, off, kind, oc.WINDOWS, cutoffs, skip, cooldown, block,
                                    REPLICATES if block == S else REPLICATES[:4], 11, target, fixed, units=units[block])
            assert same(units[block][0].sum(axis=1, dtype=np.uint64), g["counts"])   # the blocks sum to the summary's counts
            assert want["fixed_counts"].any() and want["fixed_accepts"].any() and len(set(want["fixed_counts"])) > 1
            assert np.all(want["fixed_slices"] > 0)
            if keep_short:
                assert np.all(want["sel_row"] == -1) and np.all(want["sel_cutoff"] == -1) and not want["sel_counts"].any()
            elif len(cutoffs) > 1:
                assert np.all(want["sel_row"] >= 0) and np.all(want["sel_row"] != 4) and len(set(want["sel_cutoff"])) > 1
            else:   # one cutoff: a replicate meets the target there or nowhere
                assert np.any(want["sel_row"] >= 0) and np.any(want["sel_row"] == -1) and np.all(want["sel_cutoff"] <= 0)


def check_block_borders(sm):
    """ambient tracks with S - 1, S, S + 1 and 2 S + w moving-average values at each window, one of three segments, an empty
    one and one shorter than the window, under every cooldown regime at block S and 2 S: the cooldown carries across block
    borders, the blocks of a track sum to the track's own row of mww_stream_operating_points"""
    windows = [5, 1]
    lengths, tracks = osc.boundary_tracks(np.random.default_rng(3), windows)
    n_amb = len(lengths) - 3
    # S + 1 probabilities: two blocks, the second empty at window 5 (S - 3 values) and not at window 1
    assert S + 1 in lengths[:n_amb] and 3 * S + 5 in lengths[:n_amb]
    short = [np.zeros(0, np.float32), np.full(3, 0.9, np.float32)]
    cutoffs = streaming.CUTOFFS
    crossed = 0
    for cooldown in (0, 1, 25, S + 6):
        crossed += oc.crosses_with_state(tracks[:n_amb], 5, cooldown, cutoffs[37])
        for with_short in (False, True):
            trk = (short if with_short else []) + tracks
            kind = np.array([0] * (len(trk) - 3) + [1] * 3, np.int32)
            off = np.concatenate([[0], np.cumsum([len(t) for t in trk])]).astype(np.int64)
            sm.native.set_probs(np.concatenate(trk))
            for block in (S, 2 * S):
                want, units = check_records(sm.native, trk, off, kind, windows, cutoffs, 25, cooldown, block, (65,), 5, 1e9, (1, 37))
                blk_cnt, blk_len, _ = units
                assert (np.all(want["sel_row"] == -1)) == with_short and want["fixed_counts"].any()
                first = np.concatenate([[0], np.cumsum([-(-len(t) // block) for t in trk[:len(trk) - 3]])])
                assert first[-1] == blk_cnt.shape[1] and (not with_short or (first[1] == 0 and first[2] == 1))   # the empty track has no block
                assert np.any(blk_len[0] == 0) and np.any((blk_len[0] == 0) & (blk_len[1] > 0))   # empty at window 5, not at window 1
                if block != S:
                    continue
                for j in range(len(trk) - 3):   # the track alone: its counts and its length
                    if len(trk[j]) == 0:
                        continue
                    sm.native.set_probs(trk[j])
                    counts, ma_len, _ = sm.native.operating_points(np.array([0, len(trk[j])], np.int64), np.zeros(1, np.int32), windows, cutoffs, 25, cooldown)
                    assert same(blk_cnt[:, first[j]:first[j + 1]].sum(axis=1, dtype=np.uint64), counts), (cooldown, j)
                    assert np.array_equal(blk_len[:, first[j]:first[j + 1]].sum(axis=1), ma_len[:, 0]), (cooldown, j)
                sm.native.set_probs(np.concatenate(trk))
    assert crossed >= 2   # a walk enters a later block still cooling down, at a cooldown below and at one above S
    # block 0: an empty track is a block of its own, of length 0 and without a count
    trk = short + tracks
    kind = np.array([0] * (len(trk) - 3) + [1] * 3, np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in trk])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(trk))
    _, units = check_records(sm.native, trk, off, kind, windows, cutoffs, 25, 25, 0, (65,), 5, 1e9, (1, 37))
    assert units[0].shape[1] == len(trk) - 3 and not units[0][:, 0].any() and not units[1][:, 0].any()


def check_positive_counts(sm, n_pos):
    """around the workgroup of the level kernel: 1, P - 1, P, P + 1 and 4 P + 1 positive tracks; under a skip of 25 some have
    no value at window 5 (level 0, never accepted; the window is unusable and only the fixed point carries numbers)"""
    tracks, off, kind = osc.positive_set(n_pos)
    sm.native.set_probs(np.concatenate(tracks))
    windows = [5, 1, 256, 5]
    for ignore, cutoffs in ((25, streaming.CUTOFFS), (3, np.linspace(0.0, 1.0, 128)), (3, np.array([0.37]))):
        for block in (0, S):
            g = check_surface(sm, tracks, off, kind, windows, cutoffs, ignore, 50.0, 20, 2, block, fixed=(1, len(cutoffs) // 2))
            rec = g["bootstrap"]["records"]
            assert list(g["usable"]) == [ignore == 3, True, False, ignore == 3] and (len(cutoffs) == 1 or np.all(rec["sel_row"] >= 0))
            assert np.all(rec["fixed_accepts"] <= n_pos) and (n_pos == 1 or rec["fixed_accepts"].any())
        want, _ = check_records(sm.native, tracks, off, kind, windows, cutoffs, ignore, ignore, 0, (7,), 3, 50.0, (0, 0))
        # window 5 at the smallest cutoff accepts every positive that has a value, and no other
        has_value = np.array([len(t) - ignore >= 5 for t, k in zip(tracks, kind) if k])
        draws = [streaming.bootstrap_draw(3, 1, r, np.arange(n_pos), n_pos) for r in range(7)]
        assert list(want["fixed_accepts"]) == [int(np.count_nonzero(has_value[d])) for d in draws]
        assert (ignore == 3) == bool(has_value.all())


def check_strict_comparison(sm):
    """a score equal to a cutoff is not accepted at it; a positive without a value is never accepted"""
    half = np.full(40, 0.5, np.float32)
    tracks = [half[:40], half[:30], half[:34], half[:12], half[:29], half[:0], half[:25], half[:32], half[:9]]
    kind = np.array([0, 1, 0, 1, 1, 1, 1, 0, 1], np.int32)
    off = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(tracks))
    cutoffs = np.array([-1.0, 0.25, np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), 0.75])
    for col, accepted in ((2, True), (3, False)):
        want, _ = check_records(sm.native, tracks, off, kind, [5, 3, 1], cutoffs, 10, 4, 0, (33,), 9, 1e9, (2, col))
        # positives of 30, 12, 29, 0, 25, 9 probabilities after a skip of 10: four keep a value at window 1
        draws = [streaming.bootstrap_draw(9, 1, r, np.arange(6), 6) for r in range(33)]
        assert list(want["fixed_accepts"]) == [int(np.count_nonzero(np.isin(d, (0, 1, 2, 4)))) if accepted else 0 for d in draws]
        assert np.all(want["sel_row"] == -1)   # positives without a value: no window is usable


# ---- selection
def first_crossing(faph, frr, usable, target_faph, windows=None):
    """select_operating_points with the first cutoff that meets the target in place of the rule's "and at every larger
    cutoff": what the rule is there to avoid"""
    faph, frr = np.asarray(faph, np.float64), np.asarray(frr, np.float64)
    chosen = np.full(faph.shape[0], -1, np.int64)
    for k in np.nonzero(usable)[0]:
        ok = np.nonzero(faph[k] <= target_faph)[0]
        if ok.size:
            chosen[k] = ok[0]
    windows = np.arange(chosen.size) if windows is None else np.asarray(windows, np.int64)
    best = [(frr[k, chosen[k]], faph[k, chosen[k]], int(windows[k]), k) for k in range(chosen.size) if chosen[k] >= 0]
    return chosen, (min(best)[3] if best else -1)


def selection_set():
    """Four ambient tracks of 2 S + 10 probabilities, cooldown 25, windows 1 and 2.  In three of them a value of 0.3 stands 10
    indices in front of the first block border and one of 0.9 right behind it: below 0.3 the walk accepts the first and is
    still cooling down at the second, so the second block counts 0 there and 1 at the cutoffs between; a replicate that draws
    second blocks has counts that RISE with the cutoff.  The whole track's count never rises (the greedy walk accepts the most
    candidates that a cooldown allows), only a block's does."""
    cutoffs = np.array([0.1, 0.2, 0.5, 0.8, 0.95])
    amb = [np.zeros(2 * S + 10, np.float32) for _ in range(4)]
    for j in range(3):
        amb[j][S - 10] = 0.3
        amb[j][S + 2] = 0.9
    amb[3][100:102] = 0.99   # one detection at every cutoff, at window 2 too
    pos = [np.full(40, v, np.float32) for v in (0.15, 0.45, 0.6, 0.6, 0.85, 0.97)]
    tracks = amb + pos
    kind = np.array([0] * 4 + [1] * 6, np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    return tracks, off, kind, cutoffs


def check_selection(sm):
    tracks, off, kind, cutoffs = selection_set()
    amb, pos = split(tracks, kind)
    windows = [1, 2]
    sm.native.set_probs(np.concatenate(tracks))
    units = streaming.bootstrap_units_host(amb, pos, windows, cutoffs, 25, S, 25)
    assert list(units[0][0, 1]) == [0, 0, 1, 1, 0] and list(units[0][0, 0]) == [1, 1, 0, 0, 0]   # a block's counts rise with the cutoff
    assert np.all(np.diff(units[0].sum(axis=1, dtype=np.int64), axis=1) <= 0)                       # a track's never do
    # the full data: 4 tracks of 2 S + 10 values at window 1, 4 detections at most
    hours = streaming.track_hours([2 * S + 10] * 4, STRIDE, STEP)
    one = 1 / hours
    R = 200
    # every replicate meets a target above any FAPH; none meets a negative one
    want, _ = check_records(sm.native, tracks, off, kind, windows, cutoffs, 25, 25, S, (R,), 4, 1e9, (0, 2))
    assert np.all(want["sel_row"] >= 0) and np.all(want["sel_cutoff"] == 0)
    want, _ = check_records(sm.native, tracks, off, kind, windows, cutoffs, 25, 25, S, (R,), 4, -1.0, (0, 2))
    assert np.all(want["sel_row"] == -1) and np.all(want["sel_cutoff"] == -1) and not want["sel_accepts"].any() and want["fixed_counts"].any()
    # between: a replicate that drew the 0.99 block keeps a detection at the largest cutoff and misses a target below one
    # detection per (its own) hours; the others meet it
    want, _ = check_records(sm.native, tracks, off, kind, windows, cutoffs, 25, 25, S, (R,), 4, 0.4 * one, (0, 2))
    assert np.any(want["sel_row"] == -1) and np.any(want["sel_row"] >= 0)
    # "at every larger cutoff": at a target of 1.5 detections per full hours a replicate with two second blocks and no first
    # one has 0 detections at the cutoffs 0.1 / 0.2 and 2 at 0.5 / 0.8: the first crossing is not the answer
    target = 1.5 * one
    want, _ = check_records(sm.native, tracks, off, kind, windows, cutoffs, 25, 25, S, (R,), 4, target, (0, 2))
    usable = usable_on_full_data([len(t) for t in tracks], kind, windows, 25)
    naive = streaming.bootstrap_records_host(units, usable, np.asarray(windows, np.int64), cutoffs, STRIDE, STEP, target, R, 4, (0, 2),
                                             select=first_crossing)
    differ = np.nonzero(naive["sel_cutoff"] != want["sel_cutoff"])[0]
    assert differ.size and np.all(naive["sel_cutoff"][differ] < want["sel_cutoff"][differ]) and np.all(want["sel_row"][differ] >= 0)
    assert same(naive["fixed_counts"], want["fixed_counts"])
    # the Python surface on the same set, block 0 too (whole tracks: monotone counts)
    for block in (0, S):
        check_surface(sm, tracks, off, kind, windows, cutoffs, 25, target, 50, 4, block)
    # a tie between two windows goes to the smaller window, whatever its row: silent ambient tracks, identical positives
    quiet = [np.zeros(300, np.float32), np.zeros(200, np.float32)] + [np.full(60, 0.5, np.float32)] * 3
    kind = np.array([0, 0, 1, 1, 1], np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in quiet])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(quiet))
    for windows, row in (([3, 2], 1), ([2, 3], 0), ([4, 4], 0)):
        want, _ = check_records(sm.native, quiet, off, kind, windows, streaming.CUTOFFS, 25, 25, 0, (40,), 1, 0.5, None)
        assert np.all(want["sel_row"] == row) and np.all(want["sel_cutoff"] == 0) and np.all(want["sel_accepts"] == 3)
        assert not want["fixed_counts"].any() and not want["fixed_slices"].any()   # no fixed point: zeros


def check_degenerate(sm):
    """all ambient blocks identical, all positives identical: every replicate is the full data, every interval has no width and
    sits at the point estimate"""
    rng = np.random.default_rng(8)
    a = np.clip(rng.random(700).astype(np.float32) ** 2 * 1.1, 0, 1).astype(np.float32)
    p = rng.random(80).astype(np.float32)
    tracks = [a, a, p, p, p]
    kind = np.array([0, 0, 1, 1, 1], np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(tracks))
    g = check_surface(sm, tracks, off, kind, [5, 3], streaming.CUTOFFS, 25, 30.0, 100, 6, 0)
    b = g["bootstrap"]
    r = g["recommended"]
    c = int(g["chosen"][r])
    assert r >= 0 and 0 < c and (b["fixed_row"], b["fixed_cutoff"]) == (r, c)
    rec = b["records"]
    assert np.all(rec["sel_row"] == r) and np.all(rec["sel_cutoff"] == c)
    for name in ("sel", "fixed"):
        assert np.all(rec[name + "_counts"] == g["counts"][r, c]) and np.all(rec[name + "_accepts"] == g["accepts"][r, c])
        assert np.all(rec[name + "_slices"] == 2 * (700 - int(g["windows"][r]) + 1))
    m = streaming.streaming_metrics(g)
    # two identical tracks: the summary's hours, h + h, are exactly the hours of the summed slices
    assert b["intervals"]["recall"] == b["intervals"]["recall_at_target"] == (m["streaming_recall"], m["streaming_recall"])
    assert b["intervals"]["false_accepts_per_hour"] == b["intervals"]["false_accepts_per_hour_at_target"] \
        == (m["streaming_false_accepts_per_hour"], m["streaming_false_accepts_per_hour"])


def check_intervals():
    """the percentile rule on records written by hand"""
    rec = np.zeros(40, native.BOOT_RECORD_DTYPE)
    rec["fixed_accepts"] = np.arange(40)[::-1]
    rec["fixed_counts"] = np.arange(40)
    rec["fixed_slices"] = 3600 * 50   # one hour at stride 1, step 0.02
    rec["sel_row"] = np.where(np.arange(40) < 4, -1, 0)
    rec["sel_accepts"], rec["sel_counts"], rec["sel_slices"] = 40, 2, 3600 * 50
    got = streaming.bootstrap_intervals(rec, 40, 1, 0.02, 0.9)
    # R = 40, q = 0.9: lower = v[floor(0.05 * 40)] = v[2], upper = v[ceil(0.95 * 40) - 1] = v[37]
    assert got["false_accepts_per_hour"] == (2.0, 37.0) and got["recall"] == (1 - (1 - 2 / 40), 1 - (1 - 37 / 40))
    # four replicates without a point: recall 0 and FAPH +inf, so the lower recall is 0 and the upper FAPH is infinite
    assert got["recall_at_target"] == (0.0, 1.0) and got["false_accepts_per_hour_at_target"] == (2.0, float("inf"))
    assert streaming.bootstrap_intervals(rec, 40, 1, 0.02, 0.9, fixed=False)["recall"] is None
    assert streaming.bootstrap_intervals(rec[:1], 40, 1, 0.02, 0.5)["recall"] == (1 - (1 - 39 / 40),) * 2
    for q in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="confidence"):
            streaming.bootstrap_intervals(rec, 40, 1, 0.02, q)


# ---- arguments
def check_arguments(sm):
    probs = np.linspace(0, 1, 50, dtype=np.float32)
    sm.native.set_probs(probs)
    off, kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    good = dict(windows=[5, 3], cutoffs=[0.2, 0.5], skip=3, cooldown=2, stride=1, step_s=0.02, target=5.0, replicates=8, seed=1, block=0,
                fixed=(1, 1), cap=0)

    def call(**kw):
        a = dict(good, **kw)
        return sm.native.operating_bootstrap(off, kind, a["windows"], a["cutoffs"], a["skip"], a["cooldown"], a["stride"], a["step_s"], a["target"],
                                             a["replicates"], a["seed"], a["block"], a["fixed"], a["cap"])
    before = sm.native.operating_summary(off, kind, good["windows"], good["cutoffs"], 3, 2, 1, 0.02)
    reference = call()
    bad = [dict(replicates=0), dict(replicates=native.BOOT_MAX_REPLICATES + 1), dict(replicates=-3), dict(block=1000), dict(block=-S), dict(block=S + 1),
           dict(cutoffs=[0.5, 0.2]), dict(cutoffs=[0.2, 0.2]), dict(cutoffs=[0.2, float("nan")]), dict(fixed=(2, 0)), dict(fixed=(0, 2)),
           dict(fixed=(-1, 1)), dict(fixed=(1, -1)), dict(stride=0), dict(step_s=0.0), dict(windows=[]), dict(windows=[native.OP_MAX_WINDOW + 1]),
           dict(cutoffs=[]), dict(cutoffs=np.linspace(0, 1, 129)), dict(skip=-1), dict(cooldown=-1), dict(cap=-1)]
    for b in bad:
        with pytest.raises(native.NativeError, match="error -1"):
            call(**b)
        assert sm.native.read().tobytes() == probs.tobytes()
    with pytest.raises(ValueError, match="seed"):
        call(seed=2 ** 64)
    # the scratch cap: 2 windows x 1 block x 2 cutoffs x 4 + 2 x 1 x 8 + 1 positive x 2 = 34 bytes
    assert same(call(cap=34), reference)
    with pytest.raises(native.NativeError, match="error -3.*larger block"):   # MWW_ERR_UNSUPPORTED
        call(cap=33)
    # a refused call leaves the probabilities held and what follows as they were
    assert sm.native.read().tobytes() == probs.tobytes()
    after = sm.native.operating_summary(off, kind, good["windows"], good["cutoffs"], 3, 2, 1, 0.02)
    assert all(same(x, y) for x, y in zip(before, after)) and same(call(), reference)
    lib = sm.native.nl.lib   # null pointers do not pass the wrapper: the C call itself
    vp = lambda x: x.ctypes.data_as(native.C.c_void_p)   # noqa: E731
    w, c, rec = np.array([5], np.int32), np.array([0.5]), np.zeros(3, native.BOOT_RECORD_DTYPE)
    args = [sm.native.h, vp(off), vp(kind), 2, vp(w), 1, 3, 2, vp(c), 1, 1, 0.02, 3, 7, 0, 5.0, 0, 0, 0, vp(rec)]
    for at in (0, 1, 2, 4, 8, 19):
        assert lib.mww_stream_operating_bootstrap(*[None if i == at else v for i, v in enumerate(args)]) == -1, at   # MWW_ERR_INVALID
    assert lib.mww_stream_operating_bootstrap(*args) == 0 and np.all(rec["fixed_slices"] == 16)
    # the limits: the most replicates, windows and cutoffs of the ABI; the largest seed
    recs = call(replicates=native.BOOT_MAX_REPLICATES, fixed=None)
    assert recs.shape == (native.BOOT_MAX_REPLICATES,) and same(recs[:8]["sel_row"], reference["sel_row"])
    wide = sm.native.operating_bootstrap(off, kind, [3] * native.OP_MAX_WINDOWS, np.linspace(0, 1, 128), 3, 2, 1, 0.02, 5.0, 5, 2 ** 64 - 1, 0,
                                         (native.OP_MAX_WINDOWS - 1, 127))
    tracks = [probs[:20], probs[20:]]
    units = streaming.bootstrap_units_host(tracks[:1], tracks[1:], [3] * native.OP_MAX_WINDOWS, np.linspace(0, 1, 128), 2, 0, 3)
    assert same(wide, streaming.bootstrap_records_host(units, np.ones(native.OP_MAX_WINDOWS, bool), np.full(native.OP_MAX_WINDOWS, 3), np.linspace(0, 1, 128),
                                                       1, 0.02, 5.0, 5, 2 ** 64 - 1, (native.OP_MAX_WINDOWS - 1, 127)))
    # the Python surface refuses what the restatement refuses
    for f in (lambda **kw: sm.operating_bootstrap(off, kind, [5, 3], [0.2, 0.5], 3, 1, 0.02, 5.0, **kw),
              lambda **kw: streaming.operating_bootstrap_host(tracks[:1], tracks[1:], [5, 3], [0.2, 0.5], 1, 0.02, 3, 5.0, **kw)):
        with pytest.raises(ValueError, match="confidence"):
            f(replicates=4, confidence=1.0)
    with pytest.raises(ValueError, match="block"):
        streaming.operating_bootstrap_host(tracks[:1], tracks[1:], [5, 3], [0.2, 0.5], 1, 0.02, 3, 5.0, 4, block=1000)
    with pytest.raises(ValueError, match="ascend"):
        streaming.operating_bootstrap_host(tracks[:1], tracks[1:], [5, 3], [0.5, 0.2], 1, 0.02, 3, 5.0, 4)
    with pytest.raises(ValueError, match="replicates"):
        streaming.operating_bootstrap_host(tracks[:1], tracks[1:], [5, 3], [0.2, 0.5], 1, 0.02, 3, 5.0, 0)


def check_one_kind(sm):
    rng = np.random.default_rng(4)
    tracks = [rng.random(n).astype(np.float32) for n in (300, 40, 1100)]
    off = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(tracks))
    windows = [5, 1]
    for kind, block in ((np.zeros(3, np.int32), S), (np.ones(3, np.int32), 0)):
        # the C call: no usable window, so no re-selected point; the fixed point carries what there is
        want, _ = check_records(sm.native, tracks, off, kind, windows, streaming.CUTOFFS, 25, 25, block, (9,), 2, 1e9, (1, 10))
        assert np.all(want["sel_row"] == -1)
        assert want["fixed_counts"].any() == (kind[0] == 0) and want["fixed_accepts"].any() == (kind[0] == 1)
        # the Python surface refuses as the summary does, and so does the restatement
        match = "no positive track" if kind[0] == 0 else "usable"
        with pytest.raises(ValueError, match=match):
            sm.operating_bootstrap(off, kind, windows, target_faph=1.0, replicates=4)
        with pytest.raises(ValueError, match=match):
            streaming.operating_bootstrap_host(*split(tracks, kind), windows, target_faph=1.0, replicates=4)


def check_shared_buffers(sm):
    """osc.check_shared_buffers with the bootstrap between the other entry points, sizes going large -> small -> large: every
    call returns byte for byte what it returns on a fresh stream that made only that call"""
    big = oc.inputs()
    big_kind = np.array([t % 2 for t in range(len(big.lengths))], np.int32)
    small = np.linspace(0, 1, 50, dtype=np.float32)
    small_off, small_kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    small_win = np.array([(0, 0, 60, 0, 0), (0, 2, 90, 0, 40 * 7)], native.WINDOW_DTYPE)
    boot_big = lambda st: (st.operating_bootstrap(big.off, big_kind, oc.WINDOWS, streaming.CUTOFFS, 25, 25, STRIDE, STEP, 1.0, 33, 3, S, (2, 30)),)   # noqa: E731
    boot_small = lambda st: (st.operating_bootstrap(small_off, small_kind, [5, 3], [0.2, 0.5], 3, 2, 1, 0.02, 5.0, 9, 1, 0, (1, 1)),)   # noqa: E731
    calls = [
        (big.flat, boot_big),
        (big.flat, lambda st: st.metrics(big.off, big_kind, streaming.CUTOFFS, 5, 25, 25)),
        (small, boot_small),
        (small, lambda st: st.detections(small_off, small_kind, 0.3, 3, 3, 2)),
        (big.flat, boot_big),
        (small, lambda st: st.mine(small_win, small_off, 0.3, 3, 2, 1, 1, 4)),
        (big.flat, lambda st: st.operating_summary(big.off, big_kind, oc.WINDOWS, streaming.CUTOFFS, 25, 25, STRIDE, STEP)),
        (small, boot_small),
        (big.flat, lambda st: st.operating_points(big.off, big_kind, oc.WINDOWS, streaming.CUTOFFS, 25, 25)),
        (big.flat, boot_big),
    ]
    flat = lambda out: [np.asarray(o) for o in out]   # noqa: E731
    for i, (probs, call) in enumerate(calls):
        sm.native.set_probs(probs)
        got = flat(call(sm.native))
        fresh = streaming.StreamingModel(sm.model, sm.stride, sm.mode)
        fresh.native.set_probs(probs)
        want = flat(call(fresh.native))
        fresh.native.close()
        assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), (i, got, want)
        assert any(np.frombuffer(g.tobytes(), np.uint8).any() for g in got), i


# ---- the kernels' own probabilities
def check_on(sm, off, kind, p, windows=streaming.OP_WINDOWS, ignore=25, block=0):
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    g = check_surface(sm, tracks, off, kind, windows, streaming.CUTOFFS, ignore, 1e9, 20, 5, block, stride=sm.stride)
    assert g["usable"].all() and np.all(g["bootstrap"]["records"]["sel_row"] >= 0)
    return g


def check_own_probabilities(lib, mode):
    _, sm, _, off, kind, p = dc.own_probabilities(lib, mode, lengths=(300, 120, 411, 90, 260, 120))
    check_on(sm, off, kind, p)
    check_on(sm, off, kind, p, windows=(7, 3), ignore=3, block=S)


def check_own_probabilities_q8(lib):
    """the int8 stream leaves uint8 / 255 in the buffer the bootstrap reads"""
    import q8_checks as qc
    _, model, qm = qc.make_quantized(lib, ec.DEF, 52)
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    tr = sc.Tracks(model, [300, 90, 411, 120, 260, 120], seed=21)
    off = qsm.native.run(tr.win)
    p = qsm.read_probabilities()
    assert np.array_equal(p, qsm.read_q8().astype(np.float32) * np.float32(1 / 255))
    check_on(qsm, off, np.array([0, 0, 0, 0, 1, 1], np.int32), p)
