"""Checks of mww_stream_operating_summary (csrc/tu_stream_oppoints.hip through microwakeword_amd.streaming) shared by the
emulator tests (tests/test_operating_summary_emulated.py) and the GPU tests (tests/test_operating_summary_gpu.py): the same
shapes on both.  Everything is integer or bit equality against ``mww_stream_operating_points`` (its counts; its score and
ma_len reduced on the host) and against the NumPy restatement ``streaming.operating_summary_host``; there is no tolerance.
The generators and cases of tests/operating_point_checks.py are used as they are."""
import numpy as np
import pytest

from microwakeword_amd import native, streaming
import engine_checks as ec
import operating_point_checks as oc
import stream_detect_checks as dc
import streaming_checks as sc

S = oc.S            # moving-average values per kernel segment (POST_SEG)
P = 256             # positive tracks per workgroup of the accept reduction (OPS_POS of csrc/tu_stream_oppoints.hip)
STRIDE, STEP = 3, 0.02   # hours: (n * 3) * 0.02 / 3600 has rounding in the product, the division and the sum


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_dict(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert same(got[k], want[k]), (k, got[k], want[k])
    return True


def reduced(counts, ma_len, score, kind, cutoffs, stride, step_s):
    """what the summary is defined as, from the arrays mww_stream_operating_points returns"""
    amb, pos = kind == 0, kind == 1
    cut = np.asarray(cutoffs, np.float64).reshape(-1)
    accepts = np.array([[np.count_nonzero(score[k][pos].astype(np.float64) > c) for c in cut] for k in range(score.shape[0])], np.uint64)
    hours = np.array([streaming.track_hours(ma_len[k][amb], stride, step_s) for k in range(score.shape[0])], np.float64)
    short = np.array([[np.count_nonzero(ma_len[k][amb] == 0), np.count_nonzero(ma_len[k][pos] == 0)] for k in range(score.shape[0])], np.int64)
    return counts, accepts.reshape(counts.shape), hours, short, np.array([np.count_nonzero(amb), np.count_nonzero(pos)], np.int64)


def check_equals_grid(st, off, kind, windows, cutoffs, skip, cooldown, stride=STRIDE, step_s=STEP):
    """the C call == the existing entry point reduced on the host, twice the same bytes; returns its outputs"""
    got = st.operating_summary(off, kind, windows, cutoffs, skip, cooldown, stride, step_s)
    assert [g.dtype for g in got] == [np.uint64, np.uint64, np.float64, np.int64, np.int64]
    counts, ma_len, score = st.operating_points(off, kind, windows, cutoffs, skip, cooldown)
    want = reduced(counts, ma_len, score, np.asarray(kind), cutoffs, stride, step_s)
    for name, g, w in zip(("counts", "accepts", "hours", "short_tracks", "n_kind"), got, want):
        assert same(g, w), (name, g, w)
    again = st.operating_summary(off, kind, windows, cutoffs, skip, cooldown, stride, step_s)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))
    return got


def check_equals_host(sm, tracks, off, kind, windows, cutoffs, ignore, target_faph=None, stride=STRIDE, step_s=STEP):
    """StreamingModel.operating_summary == operating_summary_host, key for key and bit for bit"""
    kind = np.asarray(kind)
    amb, pos = [tracks[t] for t in np.nonzero(kind == 0)[0]], [tracks[t] for t in np.nonzero(kind == 1)[0]]
    want = streaming.operating_summary_host(amb, pos, windows, cutoffs, stride, step_s, ignore, target_faph)
    got = sm.operating_summary(off, kind, windows, cutoffs, ignore, stride, step_s, target_faph)
    assert set(got) == set(streaming.SUMMARY_KEYS) | (set(streaming.SELECTION_KEYS) if target_faph is not None else set())
    same_dict(got, want)
    return got


def check_grid_cases(sm, case):
    """the inputs and cases of the operating-point tests: kinds interleaved, skip != cooldown, every cooldown regime"""
    cooldown, skip, parity, cutoffs = oc.CASES[case]
    inp = oc.inputs()
    n = len(inp.lengths)
    sm.native.set_probs(inp.flat)
    kind = np.array([(t + parity) % 2 for t in range(n)], np.int32)
    counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, inp.off, kind, oc.WINDOWS, cutoffs, skip, cooldown)
    assert list(n_kind) == [np.count_nonzero(kind == 0), np.count_nonzero(kind == 1)] and short.any()   # lengths 0 and 4 are in the set
    assert accepts.any() and np.all(accepts <= n_kind[1]) and hours.all()
    assert np.array_equal(accepts[2], accepts[5]) and hours[2] == hours[5]   # the repeated window
    if len(cutoffs) > 1:
        assert np.all(np.diff(accepts.astype(np.int64), axis=1) <= 0) and not accepts[:, -1].any()
    check_equals_host(sm, inp.tracks, inp.off, kind, oc.WINDOWS, cutoffs, cooldown)   # skip = cooldown: the Python surface


def boundary_tracks(rng, windows):
    """ambient tracks with S - 1, S, S + 1 moving-average values at each window, S - 1 .. S + 1 and 2 S + w probabilities, and
    one of three segments: a cooldown above S still lets a second accept in"""
    lengths = sorted({m + w - 1 for m in (S - 1, S, S + 1) for w in windows} | {S - 1, S, S + 1} | {2 * S + w for w in windows} | {3 * S + 5})
    positives = [31, 30, 60]
    return lengths + positives, dc.sweep_probabilities(lengths, rng) + dc.sweep_probabilities(positives, rng)


def check_cooldown_boundaries(sm):
    windows = [5, 1]
    lengths, tracks = boundary_tracks(np.random.default_rng(3), windows)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    kind = np.array([0] * (len(lengths) - 3) + [1] * 3, np.int32)
    sm.native.set_probs(np.concatenate(tracks))
    crossed = 0
    for cooldown in (0, 1, 25, S + 6):
        check_equals_grid(sm.native, off, kind, windows, streaming.CUTOFFS, 25, cooldown)
        # as the Python surface's skip, S + 6 leaves no positive a value: nothing to select from
        g = check_equals_host(sm, tracks, off, kind, windows, streaming.CUTOFFS, cooldown, target_faph=1e9 if cooldown <= 25 else None)
        assert g["counts"].any() and (g["usable"].all() if cooldown <= 25 else not g["usable"].any()), cooldown
        crossed += oc.crosses_with_state(tracks[:len(lengths) - 3], 5, cooldown, streaming.CUTOFFS[37])
    assert crossed >= 2   # a walk enters a later segment still cooling down, at a cooldown below and at one above S


def positive_set(n_pos, seed=9):
    """two ambient tracks of 100 / 140 probabilities between `n_pos` positives of 26..34: under a skip of 25 some keep no value
    at window 5, every one keeps one at window 1"""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(26, 35, n_pos)]
    lengths[0] = 26
    lengths.insert(min(1, n_pos), 100)
    lengths.append(140)
    kind = np.ones(len(lengths), np.int32)
    kind[min(1, n_pos)] = kind[-1] = 0
    tracks = [rng.random(n).astype(np.float32) for n in lengths]
    return tracks, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), kind


def check_positive_counts(sm, n_pos):
    """around the workgroup of the accept reduction: 1, P - 1, P, P + 1 and 4 P + 1 positive tracks"""
    tracks, off, kind = positive_set(n_pos)
    sm.native.set_probs(np.concatenate(tracks))
    windows = [5, 1, 256, 5]   # unsorted, repeated, the largest of the ABI (longer than every track)
    for ignore, cutoffs in ((25, streaming.CUTOFFS), (3, np.linspace(0.0, 1.0, 128)), (3, np.array([0.37]))):
        counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, off, kind, windows, cutoffs, ignore, ignore)
        assert list(n_kind) == [2, n_pos] and list(short[2]) == [2, n_pos] and not accepts[2].any() and hours[2] == 0
        assert accepts[1, 0] == n_pos and (short[0, 1] > 0) == (ignore == 25) and short[1].sum() == 0
        g = check_equals_host(sm, tracks, off, kind, windows, cutoffs, ignore, target_faph=50.0)
        assert list(g["usable"]) == [ignore == 3, True, False, ignore == 3] and g["n_positive"] == n_pos
        assert same(g["frr"][1], np.asarray(streaming.false_rejection_rates(
            [np.max(streaming.moving_average_in_order(p[ignore:], 1)) for p, k in zip(tracks, kind) if k], cutoffs)))


def check_strict_comparison(sm):
    """a score equal to the cutoff is rejected; a track without a value scores -inf, is counted short and never accepted"""
    half = np.full(40, 0.5, np.float32)
    tracks = [half[:40], half[:30], half[:4], half[:12], half[:29], half[:0], half[:25], half[:2], half[:9]]
    kind = np.array([0, 1, 0, 1, 1, 1, 1, 0, 1], np.int32)
    off = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(tracks))
    cutoffs = np.array([-1.0, 0.25, np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), 0.75])
    windows = [5, 3, 1]
    counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, off, kind, windows, cutoffs, 10, 4)
    # positives of 30, 12, 29, 0, 25, 9 probabilities after a skip of 10: 20, 2, 19, 0, 15, 0 left
    assert [list(r) for r in accepts] == [[3, 3, 3, 0, 0, 0], [3, 3, 3, 0, 0, 0], [4, 4, 4, 0, 0, 0]], accepts
    assert [list(r) for r in short] == [[2, 3], [1, 3], [0, 2]] and list(n_kind) == [3, 6]
    assert not counts[:, 3:].any() and counts[:, :3].all()
    for ignore in (10, 30):   # 30: no positive keeps a value
        g = check_equals_host(sm, tracks, off, kind, windows, cutoffs, ignore)
        assert not g["usable"].any() and np.isnan(g["faph"]).all() and (ignore == 10 or not g["accepts"].any())


def check_one_kind(sm):
    rng = np.random.default_rng(4)
    tracks = [rng.random(n).astype(np.float32) for n in (300, 40, 1100)]
    off = np.concatenate([[0], np.cumsum([t.size for t in tracks])]).astype(np.int64)
    sm.native.set_probs(np.concatenate(tracks))
    windows = [5, 1]
    # only ambient tracks: nothing accepted, and the Python layer refuses as the grid does
    counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, off, np.zeros(3, np.int32), windows, streaming.CUTOFFS, 25, 25)
    assert counts.any() and not accepts.any() and list(n_kind) == [3, 0] and not short.any() and hours.all()
    with pytest.raises(ValueError, match="no positive track"):
        sm.operating_summary(off, np.zeros(3, np.int32), windows)
    with pytest.raises(ValueError, match="no positive track"):
        streaming.operating_summary_host(tracks, [], windows)
    # only positive tracks: no hours, no usable window
    counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, off, np.ones(3, np.int32), windows, streaming.CUTOFFS, 25, 25)
    assert not counts.any() and accepts.any() and list(n_kind) == [0, 3] and not hours.any() and same(hours, np.zeros(2))
    g = check_equals_host(sm, tracks, off, np.ones(3, np.int32), windows, streaming.CUTOFFS, 25)
    assert not g["usable"].any() and g["n_ambient"] == 0
    with pytest.raises(ValueError, match="usable"):
        sm.operating_summary(off, np.ones(3, np.int32), windows, target_faph=1.0)


def check_validation(sm):
    """check_validation of the operating-point tests on the summary, plus stride and step_s"""
    sm.native.set_probs(np.linspace(0, 1, 50, dtype=np.float32))
    off, kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    good = dict(off=off, kind=kind, windows=[5, 3], cutoffs=[0.2, 0.5], skip=3, cooldown=2, stride=1, step_s=0.02)
    bad = [dict(off=np.array([0, 20, 51], np.int64)), dict(off=np.array([0, 30, 20], np.int64)), dict(off=np.array([-1, 20, 50], np.int64)),
           dict(skip=-1), dict(cooldown=-1), dict(windows=[]), dict(windows=[5, 0]), dict(windows=[native.OP_MAX_WINDOW + 1]),
           dict(windows=[1] * (native.OP_MAX_WINDOWS + 1)), dict(cutoffs=[]), dict(cutoffs=np.linspace(0, 1, 129)),
           dict(stride=0), dict(stride=-2), dict(step_s=0.0), dict(step_s=-0.02), dict(step_s=float("nan"))]
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(native.NativeError, match="error"):
            sm.native.operating_summary(a["off"], a["kind"], a["windows"], a["cutoffs"], a["skip"], a["cooldown"], a["stride"], a["step_s"])
    with pytest.raises(ValueError, match="offsets"):
        sm.native.operating_summary(off[:-1], kind, [5], [0.5])
    lib = sm.native.nl.lib   # null pointers do not pass the wrapper: the C call itself
    vp = lambda x: x.ctypes.data_as(native.C.c_void_p)   # noqa: E731
    w, c = np.array([5], np.int32), np.array([0.5])
    o = [np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.float64), np.zeros(2, np.int64), np.zeros(2, np.int64)]
    args = [sm.native.h, vp(off), vp(kind), 2, vp(w), 1, 3, 2, vp(c), 1, 1, 0.02] + [vp(x) for x in o]
    for at in (0, 1, 2, 4, 8, 12, 13, 14, 15, 16):
        assert lib.mww_stream_operating_summary(*[None if i == at else v for i, v in enumerate(args)]) == -1, at   # MWW_ERR_INVALID
    assert lib.mww_stream_operating_summary(*args) == 0
    assert list(o[4]) == [1, 1] and list(o[3]) == [0, 0] and o[2][0] == streaming.track_hours([16], 1, 0.02)
    # the stream is still usable, at the limits too; stride defaults to the stream's own
    got = check_equals_grid(sm.native, off, kind, [5, 3], [0.2, 0.5], 3, 2, stride=1)
    assert all(same(a, b) for a, b in zip(got, sm.native.operating_summary(off, kind, [5, 3], [0.2, 0.5], 3, 2, None, STEP)))
    counts, accepts, hours, short, n_kind = check_equals_grid(sm.native, off, kind, [native.OP_MAX_WINDOW] * native.OP_MAX_WINDOWS,
                                                              np.linspace(0, 1, 128), 3, 2)
    assert not counts.any() and not accepts.any() and not hours.any() and np.all(short == 1)


def check_shared_buffers(sm):
    """The five entry points keep their device tables in buffers of the stream that they share (csrc/stream_post.hip.h).
    Interleaved on one stream, with sizes going large -> small -> large, every call returns byte for byte what it returns on
    a fresh stream that made only that call: what a larger or a different call left in a buffer changes nothing."""
    big = oc.inputs()   # ~56 tracks up to 3001 probabilities, with the S - 1 / S / S + 1 / 2 S + 1 boundary tracks
    big_kind = np.array([t % 2 for t in range(len(big.lengths))], np.int32)
    small = np.linspace(0, 1, 50, dtype=np.float32)   # the set of check_validation
    small_off, small_kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    small_win = np.array([(0, 0, 60, 0, 0), (0, 2, 90, 0, 40 * 7)], native.WINDOW_DTYPE)
    calls = [
        (big.flat, lambda st: st.metrics(big.off, big_kind, streaming.CUTOFFS, 5, 25, 25)),
        (small, lambda st: st.detections(small_off, small_kind, 0.3, 3, 3, 2)),
        (big.flat, lambda st: st.operating_points(big.off, big_kind, oc.WINDOWS, streaming.CUTOFFS, 25, 25)),
        (small, lambda st: st.mine(small_win, small_off, 0.3, 3, 2, 1, 1, 4)),   # every track ambient
        (big.flat, lambda st: st.operating_summary(big.off, big_kind, oc.WINDOWS, streaming.CUTOFFS, 25, 25, STRIDE, STEP)),
        (big.flat, lambda st: st.detections(big.off, big_kind, 0.37, 5, 25, 25)),
        (small, lambda st: st.metrics(small_off, small_kind, [0.2, 0.5], 5, 3, 2)),
    ]
    flat = lambda out: [np.asarray(o) for o in out]   # noqa: E731  (mine also returns its detection count)
    for i, (probs, call) in enumerate(calls):
        sm.native.set_probs(probs)
        got = flat(call(sm.native))
        fresh = streaming.StreamingModel(sm.model, sm.stride, sm.mode)
        fresh.native.set_probs(probs)
        want = flat(call(fresh.native))
        fresh.native.close()
        assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), (i, got, want)
        assert any(np.frombuffer(g.tobytes(), np.uint8).any() for g in got), i   # no call of the sequence comes back empty


def check_on(sm, off, kind, p, windows=streaming.OP_WINDOWS, ignore=25, target=None):
    """the summary on the probabilities the stream holds == the grid reduced == the restatement on the probabilities read back"""
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    got = check_equals_grid(sm.native, off, kind, windows, streaming.CUTOFFS, ignore, ignore, stride=sm.stride)
    assert got[0].any() and got[1].any()
    return check_equals_host(sm, tracks, off, kind, windows, streaming.CUTOFFS, ignore, target, stride=sm.stride)


def check_own_probabilities(lib, mode):
    _, sm, _, off, kind, p = dc.own_probabilities(lib, mode)   # ambient tracks of 0 and 3 probabilities: no usable window
    assert not check_on(sm, off, kind, p)["usable"].any()
    _, sm, _, off, kind, p = dc.own_probabilities(lib, mode, lengths=(300, 120, 411, 90, 260, 120))
    g = check_on(sm, off, kind, p, target=1e9)
    assert g["usable"].all() and g["recommended"] >= 0
    check_on(sm, off, kind, p, windows=(7, 3), ignore=3)


def check_own_probabilities_q8(lib):
    """the int8 stream leaves uint8 / 255 in the buffer the summary reads"""
    import q8_checks as qc
    _, model, qm = qc.make_quantized(lib, ec.DEF, 52)
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    tr = sc.Tracks(model, [300, 90, 411, 120, 260, 120], seed=21)
    off = qsm.native.run(tr.win)
    p = qsm.read_probabilities()
    assert np.array_equal(p, qsm.read_q8().astype(np.float32) * np.float32(1 / 255))
    assert check_on(qsm, off, np.array([0, 0, 0, 0, 1, 1], np.int32), p, target=1e9)["usable"].all()
