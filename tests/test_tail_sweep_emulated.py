"""CPU-side checks of the head / dense-gradient / metric / Adam sweep (tests/tail_sweep.py): its parser and inventory against the
emulated library, the plan's coverage and stability, the input condition of every planned case, and a slice of the plan on the
emulated kernels."""
import pytest

import tail_oracle as to
import tail_sweep as ts


def test_tail_head_table_matches_the_library(emu_lib):
    """The X(C, J) list parsed from launch_head is what the library was built from: at every width of the list the block engine
    accepts exactly the final frame counts up to NRG x (largest J) (mww_block_kernels_cover: head_frame_limit), and the bf16
    modes exactly the widths HEAD_WIDTHS_BF16; the widths the list does not hold are refused by the head check."""
    table = ts.head_table()
    widths = sorted({c for c, _ in table})
    for c in (32, 48, 64):   # the last-block widths of the block-kernel table: all of them have a head
        assert c in widths
    for c in widths:
        top = max(j for cc, j in table if cc == c) * to.head_groups(c)
        for tf, want in ((1, True), (top, True), (top + 1, False)):
            ok, why = emu_lib.block_kernels_cover(frames=ts.block_frames(tf), conv1_filters=32, conv1_kernel=3, conv1_stride=1, block_filters=(c, c), block_kernel=(3, 3))
            assert ok == want and (ok or "head kernel holds at most %d" % top in why), (c, tf, why)
        ok, why = emu_lib.block_kernels_cover(frames=ts.block_frames(9, True), conv1_filters=32, conv1_kernel=3, conv1_stride=1, block_filters=(c, c), block_kernel=(5, 5),
                                              bf16=True)
        assert ok == (c in ts.HEAD_WIDTHS_BF16), (c, why)
    ok, why = emu_lib.block_kernels_cover(frames=20, conv1_filters=32, conv1_kernel=3, conv1_stride=1, block_filters=(32, 40), block_kernel=(3, 3))
    assert not ok
    assert len(ts.inventory()) == 2 * len(table) + 16 + 8
    # head_j / head_edges restate launch_head's "first entry with jmax <= J" on the parsed rows
    for c in widths:
        js, nrg = [j for cc, j in table if cc == c], to.head_groups(c)
        assert ts.head_j(c, 1) == js[0] and ts.head_j(c, nrg * js[-1]) == js[-1] and ts.head_j(c, nrg * js[-1] + 1) is None
        for prev, j in zip([0] + js, js):
            assert ts.head_edges(c, j) == (prev * nrg + 1, j * nrg)
            assert ts.head_j(c, prev * nrg + 1) == j and ts.head_j(c, j * nrg) == j
    # the ring the replay cases count on
    import os
    import re
    text = open(os.path.join(ts.ROOT, "microwakeword_amd", "csrc", "engine.hip.h")).read()
    assert int(re.search(r"constexpr int kRing = (\d+);", text).group(1)) == ts.K_RING


def test_tail_head_table_parser_fails_loudly():
    import re
    text = open(ts.MWW_LIB).read()
    m = re.search(r"X\((\d+), (\d+)\) X\((\d+), (\d+)\)", text[text.index("int launch_head("):])   # the first two rows, whatever they are
    pair = m.group(0)
    c0, j0, c1, j1 = m.groups()
    assert text.count(pair) == 1 and c0 == c1 and int(j0) < int(j1)
    with pytest.raises(ValueError, match="not a list of integers"):
        ts._parse_head_table(text.replace(pair, "X(%s, kTwo) X(%s, %s)" % (c0, c1, j1)))
    with pytest.raises(ValueError, match="cannot parse"):
        ts._parse_head_table(text.replace(pair, "Y(%s, %s) X(%s, %s)" % (c0, j0, c1, j1)))
    with pytest.raises(ValueError, match="fields"):
        ts._parse_head_table(text.replace(pair, "X(%s, %s, 1) X(%s, %s)" % (c0, j0, c1, j1)))
    with pytest.raises(ValueError, match="ascend"):
        ts._parse_head_table(text.replace(pair, "X(%s, %s) X(%s, %s)" % (c1, j1, c0, j0)))
    with pytest.raises(ValueError, match="launch_head"):
        ts._parse_head_table(text.replace("int launch_head(", "int launch_hd("))
    assert ts._parse_head_table(text) == ts.head_table()


def test_tail_sweep_covers_every_reachable_item(tmp_path):
    """uncovered() is exactly UNREACHABLE, every entry with its reason; a new instantiation in launch_head becomes required (and
    uncovered) without an edit here."""
    gap = ts.uncovered()
    assert set(gap) == set(ts.UNREACHABLE), ("not covered: %s; listed but covered: %s"
                                              % (sorted(set(gap) - set(ts.UNREACHABLE), key=str), sorted(set(ts.UNREACHABLE) - set(gap), key=str)))
    assert all(isinstance(why, str) and why for why in ts.UNREACHABLE.values())
    assert sum(k.startswith("dense_role_chunks") for k in ts.UNREACHABLE if isinstance(k, str)) == 6
    inv = ts.inventory()
    for c in ts.plan():
        names = {i for i in ts.case_items(c) if isinstance(i, str)}
        assert not names - inv, (c["id"], names - inv)
    path = tmp_path / "mww_lib.hip"
    C, J = ts.head_table()[-1]   # one more row behind the last one of the list
    last = "X(%d, %d)" % (C, J)
    text = open(ts.MWW_LIB).read()
    assert text.count(last) == 1
    path.write_text(text.replace(last, "%s X(%d, %d)" % (last, C, J + 8)))
    req = ts.required(ts.head_table(str(path)))
    assert ts.head_inst(C, J + 8, False) in req and ("edge", ts.head_inst(C, J + 8, C in ts.HEAD_WIDTHS_BF16), "lower", 2) in req
    assert ts.head_inst(C, J + 8, False) not in ts.required()
    new = [c for c in ts.plan(str(path)) if c["id"].startswith("head%dx%d" % (C, J + 8))]   # (planned from the table: storage forms x 2 edges x 3 grids)
    nrg = to.head_groups(C)
    assert len(new) == (12 if C in ts.HEAD_WIDTHS_BF16 else 6) and {c["t_final"] for c in new} == {J * nrg + 1, (J + 8) * nrg}


def test_tail_sweep_fails_on_a_flag_set_that_reaches_a_listed_form():
    """A case that launches one of the dense_role_chunks forms listed as unreachable makes uncovered() differ from UNREACHABLE."""
    cov = set()
    for c in ts.plan():
        cov |= ts.case_items(c)
    assert not cov & set(ts.UNREACHABLE)
    cov.add(ts.dense_role(False, True, False))
    assert set(ts.required()) - cov != set(ts.UNREACHABLE)


def test_tail_sweep_plan_is_stable():
    cases = ts.plan()
    ts._plan.cache_clear()
    assert ts.plan() == cases
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        assert c["B"] <= 1536 and c["T"] <= 780, ts.describe(c)
    big = [c for c in cases if c["B"] > 1057]
    assert [c["id"] for c in big] == ["head32-gstat-gridmax"]


def test_tail_sweep_ratios_keep_nan():
    """A NaN or inf error is an error without bound whatever was recorded before or after it; so is a NaN bound."""
    for bad in (float("nan"), float("inf")):
        r = ts.Ratios()
        r.add("x", [0.0, 0.5], [1.0, 1.0])
        r.add("x", [0.0, bad], [1.0, 1.0])
        r.add("x", [0.0, 0.1], [1.0, 1.0])
        assert r["x"] == float("inf")
        with pytest.raises(AssertionError):
            r.check(ts.plan()[0])
    r = ts.Ratios()
    r.add("x", [1.0], [float("nan")])
    assert r["x"] == float("inf")
    r = ts.Ratios()
    r.add("x", [0.0, 0.5], [0.0, 1.0])
    assert r["x"] == 0.5
    with pytest.raises(AssertionError, match="holds a NaN"):
        ts._finite(ts.plan()[0], gradient=[1.0, float("nan")])


PLAN = ts.plan()


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_tail_sweep_input_condition(case):
    """From the float64 oracle alone, for every planned case (the GPU-only ones included): dropping the largest term of any one
    final frame row moves z by more than twice its bound in some window, dropping any one window moves some dense-gradient
    element by more than twice its bound."""
    cond = ts.input_condition(case)
    if cond is None:
        assert case["kind"] in ("metric-edge", "partials", "cumulative", "adam-apply", "mixconv", "graph-whole-step")
        return
    rows, windows = cond
    assert len(rows) == 0 and len(windows) == 0, (ts.describe(case), rows, windows)


SLICE = ts.emulator_slice()


def test_tail_sweep_slice_holds_every_route():
    got = set()
    for c in SLICE:
        got |= {i for i in ts.case_items(c) if isinstance(i, str) and not i.startswith("head_kernel")}
    want = {i for i in ts.inventory() - set(ts.UNREACHABLE) if not i.startswith("head_kernel")}
    assert got == want, (want - got, got - want)
    heads = {i for c in SLICE for i in ts.case_items(c) if isinstance(i, str) and i.startswith("head_kernel")}
    table = ts.head_table()
    for C in sorted({c for c, _ in table}):   # the smallest and the largest J of every width, as the table has them
        js = [j for c, j in table if c == C]
        assert {ts.head_inst(C, js[0], False), ts.head_inst(C, js[-1], False)} <= heads


@pytest.mark.parametrize("case", SLICE, ids=[c["id"] for c in SLICE])
def test_tail_sweep_slice(emu_lib, case):
    ts.run_case(emu_lib, case)
