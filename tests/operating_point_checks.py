"""Checks of mww_stream_operating_points (csrc/tu_stream_oppoints.hip through microwakeword_amd.streaming) shared by the
emulator tests (tests/test_operating_points_emulated.py) and the GPU tests (tests/test_operating_points_gpu.py): the same
shapes on both.  Everything is integer or bit equality against ``mww_stream_metrics`` at each window and against the NumPy
restatement ``streaming.operating_points_host``; there is no tolerance."""
import numpy as np
import pytest

from microwakeword_amd import native, streaming
import engine_checks as ec
import stream_detect_checks as dc
import streaming_checks as sc

S = 1024   # moving-average values per kernel segment (POST_SEG of csrc/stream_post.hip.h)
assert S == dc.SEG   # sweep_lengths places its boundary tracks around the detect kernel's segment: the same size

WINDOWS = (1, 2, 5, 10, 256, 5)   # unsorted tail, a repeat, the largest window of the ABI
# (cooldown, skip, kind parity, cutoffs): every cooldown and both skips under the 101 cutoffs, the kinds swapped from case to
# case - the cooldown acts on ambient tracks only, the skip on positive tracks only -, then the largest and smallest cutoff
# counts.  S - 1 is the largest state a segment tabulates, S + 1 and 2 S + 500 make the walk skip whole segments.
CASES = {
    "cd0": (0, 0, 0, streaming.CUTOFFS),
    "cd1": (1, 25, 1, streaming.CUTOFFS),
    "cd25": (25, 25, 0, streaming.CUTOFFS),
    "cdS-1": (S - 1, 0, 1, streaming.CUTOFFS),
    "cdS+1": (S + 1, 25, 0, streaming.CUTOFFS),
    "cd2S+500": (2 * S + 500, 0, 1, streaming.CUTOFFS),
    "cd25_swapped": (25, 0, 1, streaming.CUTOFFS),
    "128cutoffs": (25, 25, 1, np.linspace(0.0, 1.0, 128)),
    "1cutoff": (25, 25, 0, np.array([0.37])),
}


class Inputs:
    """the probability set of the detection sweep (40 tracks) plus tracks whose moving average has S - 1, S, S + 1 and
    2 S + 1 values at the smallest and the largest window, without and with the skip of a positive track"""

    def __init__(self, seed=11):
        rng = np.random.default_rng(seed)
        lengths = dc.sweep_lengths(rng)
        assert len(lengths) == 40 and max(lengths) <= 3001
        extra = sorted({m + w - 1 + sk for m in (S - 1, S, S + 1, 2 * S + 1) for w in (min(WINDOWS), max(WINDOWS)) for sk in (0, 25)}
                       - set(lengths))
        self.lengths = lengths + extra
        self.tracks = dc.sweep_probabilities(lengths, rng) + dc.sweep_probabilities(extra, rng)
        self.flat = np.concatenate(self.tracks)
        self.off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)


_inputs = []


def inputs():
    if not _inputs:
        _inputs.append(Inputs())
    return _inputs[0]


def crosses_with_state(tracks, window, cooldown, cutoff):
    """does some track's walk enter a later segment while still cooling down (a non-zero entry state)?"""
    for p in tracks:
        ma = streaming.moving_average_in_order(p, window)
        for i in streaming.detection_positions([ma], cutoff, cooldown)[0]:
            nxt = int(i) + max(cooldown, 1)
            if nxt < ma.size and nxt // S > int(i) // S and nxt % S:
                return True
    return False


def check_grid(sm, case):
    cooldown, skip, parity, cutoffs = CASES[case]
    inp = inputs()
    n = len(inp.lengths)
    sm.native.set_probs(inp.flat)
    kind = np.array([(t + parity) % 2 for t in range(n)], np.int32)
    counts, ma_len, score = sm.native.operating_points(inp.off, kind, WINDOWS, cutoffs, skip, cooldown)
    assert counts.shape == (len(WINDOWS), len(cutoffs)) and counts.dtype == np.uint64
    assert ma_len.shape == (len(WINDOWS), n) and ma_len.dtype == np.int64 and score.shape == (len(WINDOWS), n) and score.dtype == np.float32
    # row k is mww_stream_metrics at windows[k]: the integers, the score bits
    for k, w in enumerate(WINDOWS):
        m_counts, m_len, m_score = sm.native.metrics(inp.off, kind, cutoffs, w, skip, cooldown)
        assert np.array_equal(counts[k], m_counts), (case, w, counts[k], m_counts)
        assert np.array_equal(ma_len[k], m_len), (case, w)
        assert score[k].tobytes() == m_score.tobytes(), (case, w)
    # ... and the host restatement
    amb, pos = np.nonzero(kind == 0)[0], np.nonzero(kind == 1)[0]
    host = streaming.operating_points_host([inp.tracks[t] for t in amb], [inp.tracks[t] for t in pos], WINDOWS, cutoffs,
                                           ignore_slices_after_accept=cooldown, skip=skip)
    assert np.array_equal(counts, host["counts"]), (case, counts, host["counts"])
    assert np.array_equal(ma_len[:, amb], host["ambient_ma_len"]) and np.array_equal(ma_len[:, pos], host["positive_ma_len"]), case
    assert score[:, pos].tobytes() == host["score"].tobytes() and not score[:, amb].any(), case
    # two calls, the same bytes
    again = sm.native.operating_points(inp.off, kind, WINDOWS, cutoffs, skip, cooldown)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (counts, ma_len, score))), case
    # what the inputs are for, judged on the restatement
    want = host["counts"]
    assert any(not np.array_equal(want[0], want[k]) for k in range(1, len(WINDOWS))), case
    assert np.array_equal(want[2], want[5])   # the repeated window
    if len(cutoffs) > 1:
        assert not want[:, -1].any(), case   # no average is above 1.0: a column of zeros
    if cooldown == 25 and len(cutoffs) == 101:
        c = 37
        candidates = sum(int(np.count_nonzero(streaming.moving_average_in_order(inp.tracks[t], 5).astype(np.float64) > cutoffs[c])) for t in amb)
        assert candidates > int(want[2, c]) > 0, (case, candidates, want[2, c])   # the cooldown suppresses candidates
        assert crosses_with_state([inp.tracks[t] for t in amb], 5, cooldown, cutoffs[c]), case


def check_validation(sm):
    sm.native.set_probs(np.linspace(0, 1, 50, dtype=np.float32))
    off, kind = np.array([0, 20, 50], np.int64), np.array([0, 1], np.int32)
    good = dict(off=off, kind=kind, windows=[5, 3], cutoffs=[0.2, 0.5], skip=3, cooldown=2)
    bad = [dict(off=np.array([0, 20, 51], np.int64)), dict(off=np.array([0, 30, 20], np.int64)), dict(off=np.array([-1, 20, 50], np.int64)),
           dict(skip=-1), dict(cooldown=-1), dict(windows=[]), dict(windows=[5, 0]), dict(windows=[native.OP_MAX_WINDOW + 1]),
           dict(windows=[1] * (native.OP_MAX_WINDOWS + 1)), dict(cutoffs=[]), dict(cutoffs=np.linspace(0, 1, 129))]
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(native.NativeError, match="error"):
            sm.native.operating_points(a["off"], a["kind"], a["windows"], a["cutoffs"], a["skip"], a["cooldown"])
    lib = sm.native.nl.lib   # null pointers do not pass the wrapper: the C call itself
    vp = lambda x: x.ctypes.data_as(native.C.c_void_p)   # noqa: E731
    w, c = np.array([5], np.int32), np.array([0.5])
    o1, o2, o3 = np.zeros(1, np.uint64), np.zeros(2, np.int64), np.zeros(2, np.float32)
    args = [sm.native.h, vp(off), vp(kind), 2, vp(w), 1, 3, 2, vp(c), 1, vp(o1), vp(o2), vp(o3)]
    for at in (0, 1, 2, 4, 8, 10, 11, 12):
        assert lib.mww_stream_operating_points(*[None if i == at else v for i, v in enumerate(args)]) == -1, at   # MWW_ERR_INVALID
    assert lib.mww_stream_operating_points(*args) == 0
    # the stream is still usable, at the limits too
    counts, ma_len, score = sm.native.operating_points(off, kind, [5, 3], [0.2, 0.5], 3, 2)
    for k, win in enumerate((5, 3)):
        m = sm.native.metrics(off, kind, [0.2, 0.5], win, 3, 2)
        assert np.array_equal(counts[k], m[0]) and np.array_equal(ma_len[k], m[1]) and score[k].tobytes() == m[2].tobytes()
    assert counts[0, 0] > 0 and list(ma_len[0]) == [16, 23]
    counts, ma_len, score = sm.native.operating_points(off, kind, [native.OP_MAX_WINDOW] * native.OP_MAX_WINDOWS, np.linspace(0, 1, 128), 3, 2)
    assert not counts.any() and not ma_len.any() and np.all(score[:, 0] == 0) and np.all(np.isneginf(score[:, 1]))


def check_on(sm, off, kind, p, windows=streaming.OP_WINDOWS, ignore=25):
    """the grid on the probabilities the stream holds == metrics per window == the restatement on the probabilities read back"""
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    amb, pos = np.nonzero(kind == 0)[0], np.nonzero(kind == 1)[0]
    host = streaming.operating_points_host([tracks[t] for t in amb], [tracks[t] for t in pos], windows, ignore_slices_after_accept=ignore)
    counts, ma_len, score = sm.operating_points(off, kind, windows, ignore_slices_after_accept=ignore)
    assert np.array_equal(counts, host["counts"]) and counts.any(), (counts, host["counts"])
    assert np.array_equal(ma_len[:, amb], host["ambient_ma_len"]) and np.array_equal(ma_len[:, pos], host["positive_ma_len"])
    assert score[:, pos].tobytes() == host["score"].tobytes()
    for k, w in enumerate(windows):
        m = sm.metrics(off, kind, streaming.CUTOFFS, w, ignore)
        assert np.array_equal(counts[k], m[0]) and np.array_equal(ma_len[k], m[1]) and score[k].tobytes() == m[2].tobytes(), w


def check_own_probabilities(lib, mode):
    _, sm, _, off, kind, p = dc.own_probabilities(lib, mode)
    check_on(sm, off, kind, p)
    check_on(sm, off, kind, p, windows=(7, 3), ignore=3)


def check_own_probabilities_q8(lib):
    """the int8 stream leaves uint8 / 255 in the buffer the grid reads"""
    import q8_checks as qc
    _, model, qm = qc.make_quantized(lib, ec.DEF, 52)
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    tr = sc.Tracks(model, [300, 0, 411, 3, 260, 120], seed=21)
    off = qsm.native.run(tr.win)
    p = qsm.read_probabilities()
    assert np.array_equal(p, qsm.read_q8().astype(np.float32) * np.float32(1 / 255))
    check_on(qsm, off, np.array([0, 0, 0, 0, 1, 1], np.int32), p)


def check_selection_rule():
    sel = streaming.select_operating_points
    frr = np.array([[0.0, 0.1, 0.2, 0.3, 0.4]] * 3)
    yes = np.ones(3, bool)
    # a non-monotone row: 0.4 at cutoff 1 is a first crossing, but cutoff 2 is above the target again
    faph = np.array([[3.0, 0.4, 0.9, 0.5, 0.0], [3.0, 2.0, 0.5, 0.2, 0.0], [3.0, 2.0, 1.0, 0.8, 0.6]])
    chosen, rec = sel(faph, frr, yes, 0.5)
    assert list(chosen) == [3, 2, -1] and rec == 1   # row 2 never meets the target; FRR 0.2 beats 0.3
    chosen, rec = sel(faph, frr, yes, 0.1)
    assert list(chosen) == [4, 4, -1] and rec == 0   # equal FRR and FAPH: the smaller window (the earlier row)
    assert sel(faph, frr, yes, 0.1, windows=[7, 3, 5])[1] == 1   # ... by size, not by row
    assert sel(faph, frr, yes, 0.1, windows=[4, 4, 4])[1] == 0
    # a tie in FRR goes to the smaller FAPH
    faph2 = np.array([[3.0, 0.5, 0.5, 0.5, 0.0], [3.0, 0.3, 0.3, 0.3, 0.0], [3.0, 0.3, 0.3, 0.3, 0.0]])
    chosen, rec = sel(faph2, frr, yes, 0.5)
    assert list(chosen) == [1, 1, 1] and rec == 1
    assert sel(faph2, frr, yes, 0.5, windows=[3, 9, 4])[1] == 2   # then to the smaller window
    # no window meets the target: no recommendation; the boundary counts (<=)
    chosen, rec = sel(np.full((2, 3), 2.0), frr[:2, :3], yes[:2], 1.0)
    assert list(chosen) == [-1, -1] and rec == -1
    assert list(sel(np.full((2, 3), 1.0), frr[:2, :3], yes[:2], 1.0)[0]) == [0, 0]
    # an unusable window is left out, even where its numbers would win
    chosen, rec = sel(np.array([[0.0] * 5, faph[1], faph[0]]), np.array([[0.0] * 5, frr[1], frr[0]]), np.array([False, True, True]), 0.5)
    assert list(chosen) == [-1, 2, 3] and rec == 1
    with pytest.raises(ValueError, match="usable"):
        sel(faph, frr, np.zeros(3, bool), 0.5)
    # through the host restatement: window 40 is longer than the second ambient track, window 30 leaves the positive nothing
    rng = np.random.default_rng(5)
    amb = [rng.random(400).astype(np.float32), rng.random(39).astype(np.float32)]
    pos = [rng.random(54).astype(np.float32), np.ones(200, np.float32)]
    g = streaming.operating_points_host(amb, pos, (5, 40, 30, 2), target_faph=400.0)
    assert list(g["usable"]) == [True, False, False, True] and g["recommended"] in (0, 3) and list(g["chosen"][1:3]) == [-1, -1]
    assert np.isnan(g["faph"][1]).all() and np.isnan(g["chosen_cutoff"][1]) and g["chosen_cutoff"][0] == g["cutoffs"][g["chosen"][0]]
    want = sel(g["faph"], g["frr"], g["usable"], 400.0, g["windows"])
    assert list(want[0]) == list(g["chosen"]) and want[1] == g["recommended"]
    text = streaming.operating_point_text(g).splitlines()
    assert len(text) == 5 and "unusable" in text[1] and "unusable" in text[2] and text[4].startswith("Recommended: window %d," % g["windows"][g["recommended"]])
    r = g["recommended"]
    assert streaming.operating_point_settings(g, "stream", True) == {
        "probability_cutoff": float(g["chosen_cutoff"][r]), "sliding_window_size": int(g["windows"][r]),
        "false_accepts_per_hour": float(g["faph"][r, g["chosen"][r]]), "false_rejection_rate": float(g["frr"][r, g["chosen"][r]]),
        "target_false_accepts_per_hour": 400.0, "mode": "stream", "quantized": True}
    with pytest.raises(ValueError, match="usable"):
        streaming.operating_points_host(amb, pos, (40, 64), target_faph=1.0)
