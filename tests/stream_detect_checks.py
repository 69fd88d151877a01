"""Checks of mww_stream_detections (csrc/tu_stream_detect.hip through microwakeword_amd.streaming) shared by the emulator
tests (tests/test_stream_detect_emulated.py) and the GPU tests (tests/test_stream_detect_gpu.py): the same shapes on both.
Everything here is integer or bit equality against the NumPy restatement ``streaming.detection_positions`` on the explicit
in-order float32 moving average; the only tolerance is streaming_checks.PROB_TOL in the closed loop through the model."""
import itertools

import numpy as np

from microwakeword_amd import native, streaming
import engine_checks as ec
import streaming_checks as sc

SEG = 1024   # moving-average values per kernel segment (POST_SEG of csrc/stream_post.hip.h)

WINDOWS, COOLDOWNS, SKIPS, CUTOFFS = (1, 5), (0, 1, 25), (0, 25), (0.0, 0.5, 0.37, 1.0)


def sweep_lengths(rng):
    """~40 track lengths: the edge cases of the window and skip, and moving-average lengths SEG - 1, SEG, SEG + 1 (and
    2 SEG) for either window, without and with the skip of a positive track"""
    fixed = [0, 4, 5, 6, 30, 255, 256, 257, 1000, 3001]
    around = sorted({SEG + w - 1 + sk + d for w in WINDOWS for sk in SKIPS for d in (-1, 0, 1)}            # 12 lengths
                    | {2 * SEG + w - 1 + d for w in WINDOWS for d in (-1, 0, 1)})                         # 6 lengths
    return fixed + around + [int(v) for v in rng.integers(1, 3000, 12)]


def sweep_probabilities(lengths, rng):
    probs = [np.clip(rng.random(n).astype(np.float32) ** 2 * 1.1, 0, 1).astype(np.float32) for n in lengths]
    up = lambda v: np.nextafter(np.float32(v), np.float32(2))   # noqa: E731
    big = [i for i, n in enumerate(lengths) if n >= 1000]
    # runs of values equal to a cutoff and one ulp above it (strict '>'), all ones, all zeros, across a segment boundary
    for j, i in enumerate(big):
        p, n = probs[i], lengths[i]
        pick = j % 7
        if pick == 0:
            p[10:400] = np.float32(0.37)
            p[400:700] = up(0.37)
        elif pick == 1:
            p[5:300] = np.float32(0.5)
            p[300:n - 3] = up(0.5)
        elif pick == 2:
            p[:] = np.float32(1.0)
        elif pick == 3:
            p[:n // 2] = np.float32(0.0)
            p[n // 2:] = up(0.0)
        elif pick == 4:
            p[SEG - 40:min(n, SEG + 40)] = np.float32(0.99)
    return probs


class Oracle:
    """the restatement of one probability set, cached per parameter (the device runs every combination)"""

    def __init__(self, tracks):
        self.tracks = tracks
        self._ma, self._pos = {}, {}

    def ma(self, t, window, skip):
        key = (t, window, skip)
        if key not in self._ma:
            self._ma[key] = streaming.moving_average_in_order(self.tracks[t][skip:], window)
        return self._ma[key]

    def positions(self, t, window, cooldown, cutoff):
        key = (t, window, cooldown, cutoff)
        if key not in self._pos:
            self._pos[key] = streaming.detection_positions([self.ma(t, window, 0)], cutoff, cooldown)[0]
        return self._pos[key]


def expected(oracle, kind, window, skip, cooldown, cutoff):
    ev, count, best, score = [], [], [], []
    for t, k in enumerate(kind):
        if k == 0:
            ma = oracle.ma(t, window, 0)
            at = oracle.positions(t, window, cooldown, cutoff)
            ev += [(t, int(i), ma[i]) for i in at]
            count.append(at.size)
            best.append(-1)
            score.append(np.float32(0))
        else:
            ma = oracle.ma(t, window, skip)
            count.append(0)
            best.append(int(np.argmax(ma)) if ma.size else -1)   # argmax: the first index that attains the maximum
            score.append(np.max(ma) if ma.size else np.float32(-np.inf))
    return (np.array(ev, native.DETECTION_DTYPE).reshape(-1), np.array(count, np.int64), np.array(best, np.int64),
            np.array(score, np.float32))


def same_events(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


def check_against_restatement(sm, seed=11):
    rng = np.random.default_rng(seed)
    lengths = sweep_lengths(rng)
    assert {SEG - 1, SEG, SEG + 1} <= set(lengths) and len(lengths) == 40
    probs = sweep_probabilities(lengths, rng)
    flat = np.concatenate(probs)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    sm.native.set_probs(flat)
    oracle = Oracle(probs)
    most, suppressed, empty = 0, 0, 0
    # the sweep, then cooldowns that reach the segment size: the walk's state then spans whole segments
    cases = list(itertools.product(WINDOWS, COOLDOWNS, SKIPS, CUTOFFS)) + [(1, SEG - 1, 0, 0.0), (5, SEG, 25, 0.37), (1, SEG + 1, 0, 0.5), (1, 2500, 0, 0.0)]
    for window, cooldown, skip, cutoff in cases:
        # every length is ambient under half of the cutoffs and positive under the other half
        kind = np.array([(t + CUTOFFS.index(cutoff)) % 2 for t in range(len(lengths))], np.int32)
        what = dict(window=window, cooldown=cooldown, skip=skip, cutoff=cutoff)
        want_ev, want_count, want_best, want_score = expected(oracle, kind, window, skip, cooldown, cutoff)
        ev, count, best, score = sm.native.detections(off, kind, cutoff, window, skip, cooldown)
        assert same_events(ev, want_ev), (what, ev[:5], want_ev[:5], ev.size, want_ev.size)
        assert np.array_equal(count, want_count), (what, count, want_count)
        assert np.array_equal(best, want_best), (what, best, want_best)
        assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32)), (what, score, want_score)
        m_counts, _, m_score = sm.native.metrics(off, kind, [cutoff], window, skip, cooldown)
        assert int(m_counts[0]) == int(count.sum()), (what, m_counts, count.sum())
        pos = kind == 1
        assert np.array_equal(score[pos].view(np.uint32), m_score[pos].view(np.uint32)), what
        # a capacity that is too small: the full count, the exact prefix
        cap = ev.size // 2
        ev2, count2, best2, score2 = sm.native.detections(off, kind, cutoff, window, skip, cooldown, capacity=cap)
        assert same_events(ev2, ev[:cap]) and np.array_equal(count2, count), what
        # two runs, the same bytes
        ev3, count3, best3, score3 = sm.native.detections(off, kind, cutoff, window, skip, cooldown)
        assert ev3.tobytes() == ev.tobytes() and count3.tobytes() == count.tobytes() and best3.tobytes() == best.tobytes() \
            and score3.tobytes() == score.tobytes(), what
        # what this case exercised, judged on the restatement
        most = max(most, int(want_count.sum()))
        empty += int(want_count.sum() == 0)
        candidates = sum(int(np.count_nonzero(oracle.ma(t, window, 0).astype(np.float64) > cutoff)) for t in np.nonzero(kind == 0)[0])
        suppressed += int(candidates > int(want_count.sum()))
    assert most > 100 and suppressed >= 1 and empty >= 1, (most, suppressed, empty)


def check_validation(sm):
    sm.native.set_probs(np.linspace(0, 1, 50, dtype=np.float32))
    off, kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    bad = [dict(off=np.array([0, 20, 51], np.int64)), dict(off=np.array([0, 30, 20], np.int64)), dict(window=0), dict(skip=-1),
           dict(cooldown=-1), dict(kind=np.array([0, 2], np.int32))]
    for b in bad:
        a = dict(dict(off=off, kind=kind, cutoff=0.5, window=5, skip=3, cooldown=2), **b)
        try:
            sm.native.detections(a["off"], a["kind"], a["cutoff"], a["window"], a["skip"], a["cooldown"])
        except native.NativeError as e:
            assert "error" in str(e)
        else:
            raise AssertionError("accepted %r" % (b,))
    ev, count, best, score = sm.native.detections(off, kind, 0.2, 5, 3, 2)
    assert count[1] == 0 and best[0] == -1 and score[0] == 0 and best[1] == 50 - 20 - 3 - 5 and ev.size == count[0] > 0


def own_probabilities(lib, mode, lengths=(300, 0, 411, 3, 260, 120), n_amb=4, quantized=False):
    """DEF at T = 52 over sc.Tracks: (model, streaming model, tracks, offsets, kind, probabilities)"""
    flags, T = ec.DEF, 52
    _, model = sc.make_model(lib, flags, T)
    sm = streaming.StreamingModel(model, int(flags["stride"]), mode)
    tr = sc.Tracks(model, list(lengths), seed=21)
    off = sm.native.run(tr.win)
    kind = np.array([0] * n_amb + [1] * (len(lengths) - n_amb), np.int32)
    return model, sm, tr, off, kind, sm.read_probabilities()


def median_cutoff(p, off, window=5):
    mas = [streaming.moving_average_in_order(p[off[t]:off[t + 1]], window) for t in range(off.size - 1)]
    return float(np.median(np.concatenate(mas))), mas


def check_positions_on(sm, off, kind, p, window=5, cooldown=25):
    """detections on the probabilities the stream holds == the restatement on the probabilities read back"""
    cutoff, _ = median_cutoff(p, off, window)
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    want = expected(Oracle(tracks), kind, window, cooldown, cooldown, cutoff)
    got = sm.detections(off, kind, cutoff, window, cooldown)
    assert same_events(got[0], want[0]), (got[0], want[0])
    assert got[0].size > 0
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(g, w), (g, w)
    return cutoff, got


def check_own_probabilities(lib, mode):
    _, sm, _, off, kind, p = own_probabilities(lib, mode)
    check_positions_on(sm, off, kind, p)
    check_positions_on(sm, off, kind, p, window=5, cooldown=3)


def check_own_probabilities_q8(lib):
    """the int8 stream leaves uint8 / 255 in the buffer the detections read"""
    import q8_checks as qc
    _, model, qm = qc.make_quantized(lib, ec.DEF, 52)
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    tr = sc.Tracks(model, [300, 0, 411, 3, 260, 120], seed=21)
    off = qsm.native.run(tr.win)
    p = qsm.read_probabilities()
    assert np.array_equal(p, qsm.read_q8().astype(np.float32) * np.float32(1 / 255))
    check_positions_on(qsm, off, np.array([0, 0, 0, 0, 1, 1], np.int32), p)


def check_clips_closed_loop(lib):
    """non_stream mode: a detection's clip is the window that produced the last probability of its average"""
    T, w = 52, 5
    model, sm, tr, off, kind, p = own_probabilities(lib, "non_stream", lengths=(300, 60, 411, 52, 260), n_amb=5)
    cutoff, (ev, _, _, _) = check_positions_on(sm, off, kind, p, window=w, cooldown=3)
    clips, kept = streaming.detection_clips(tr.win, ev, T, 1, "non_stream", w, return_kept=True)
    assert kept.size == ev.size and np.all(clips["copy_rows"] == T) and ev.size >= 8   # no padding: every clip is a full window
    x = []
    for s in range(0, clips.size, model.engine.max_batch):
        c = clips[s:s + model.engine.max_batch]
        model.engine.assemble(c, None, 0, 0)
        x.append(model.engine.get_batch(c.size))
    x = np.concatenate(x)
    n = ev["index"] + w - 1
    for j in range(ev.size):
        t, e = int(ev["track"][j]), T + int(n[j])
        assert np.array_equal(x[j], tr.frames[t][e - T:e]), j
    pm = np.concatenate([model.predict_on_batch(x[s:s + 64]).reshape(-1) for s in range(0, x.shape[0], 64)])
    err = np.abs(pm - p[off[ev["track"]] + n]).max()
    assert err <= sc.PROB_TOL, err
    # context rows, and a padded track: rows that exist in no store are subtracted and clipped
    more = streaming.detection_clips(tr.win, ev, T, 1, "non_stream", w, before=7, after=4)
    lo = np.maximum(n - 7, 0)
    hi = np.minimum(T + n + 4, np.asarray(tr.lengths)[ev["track"]])
    assert np.array_equal(more["copy_rows"], hi - lo) and np.array_equal(more["src_elem"], tr.win["src_elem"][ev["track"]] + lo * 40)
    padded = np.array([(0, 10, 90, 0, 400)], native.WINDOW_DTYPE)
    fake = np.array([(0, 0, 0.9), (0, 1, 0.9), (0, 20, 0.9)], native.DETECTION_DTYPE)
    c = streaming.detection_clips(padded, fake, T, 1, "stream", 5, before=0, after=0)   # outputs 4, 5, 24 -> rows end at 5, 6, 25
    assert c.size == 1 and c["copy_rows"][0] == 15 and c["src_elem"][0] == 400   # the first two lie inside the padding
    c = streaming.detection_clips(padded, fake, 4, 2, "stream", 5)   # stride 2: output n ends at row 2 (n + 1)
    assert list(c["copy_rows"]) == [2, 4] and list(c["src_elem"]) == [400, 400 + 36 * 40]
