"""CPU-side checks of the conv/BN graph kernel sweep (tests/graph_table_sweep.py): its inventory against the emulated library,
the plan's coverage, stability and conditioning, and a slice of the plan on the emulated kernels with the route check."""
import collections

import pytest

import engine_checks as ec
import graph_table_sweep as gts
from microwakeword_amd import native
from microwakeword_amd.layout import GraphMixedNetLayout


def _refusal(lib, width):
    """None when a one-block MixedNet of that pointwise width is accepted by the graph engine, else the library's message."""
    lay = GraphMixedNetLayout(gts._mixednet_flags(16, [width], [[3]]), 40)
    try:
        native.Engine(lib=lib, **lay.engine_args(2)).close()
    except native.NativeError as e:
        return str(e)
    return None


def test_graph_table_inventory_matches_the_library(emu_lib):
    """The tables parsed from graph_launch.hip.h are what the library was built from: over a candidate space wider than the table
    (even widths 4..72) a one-block probe is accepted exactly for the widths of MWW_G_WIDTHS, every other one refused as not
    instantiated; the inventory holds the number of instantiations per launcher that the tables give."""
    t = gts.tables()
    assert t["widths"] == (8, 10, 12, 16, 20, 24, 30, 32, 36, 40, 48, 60, 64)
    for w in range(4, 73, 2):
        why = _refusal(emu_lib, w)
        if w in t["widths"]:
            assert why is None, (w, why)
        else:
            assert why is not None and "not instantiated" in why, (w, why)
    assert (len(t["shapes"]), len(t["pairs"]), sorted(t["twins"])) == (11, 15, [8, 10, 12, 16, 20, 24, 32])
    for key in ("fwd", "fwd2", "wg", "xg", "bwd", "bwd2"):
        assert all(r[0] in t["shapes"] for r in t[key]), key   # every list entry names a declared shape
    inv = gts.inventory()
    count = collections.Counter(i.split("<")[0] for i in inv)
    assert count["gconv_kernel"] == 2 * 13 + 12 and count["gconv_chunk_kernel"] == 2 * 13
    assert count["gconv_wgrad_kernel"] == 13 + 1 and count["gconv_wgrad_chunk_kernel"] == 13
    assert count["gconv_bwd_kernel"] == 15 + 11 and count["gconv_bwd_chunk_kernel"] == 15
    assert count["gconv_fwd2_kernel"] == 7 + 4 and count["gconv_bwd2_kernel"] == 7 + 4
    assert count["gconv_xg_kernel"] == 1 and count["gconv_wgrad_xg_kernel"] == 1 and count["gdw_kernel"] == 2
    assert len(inv) == sum(count.values()) == 167


def test_graph_table_parser_fails_loudly():
    text = open(gts.LAUNCH_H).read()
    with pytest.raises(ValueError, match="MWW_G_TWIN_WIDTHS"):
        gts._parse_tables(text.replace("#define MWW_G_TWIN_WIDTHS(X) X(8)", "#define MWW_G_TWINS(X) X(8)"))
    with pytest.raises(ValueError, match="MWW_G_BWD_PAIRS"):
        gts._parse_tables(text.replace("X(30, 24) X(10, 10)", "X(30, 24) X(10, kTen)"))
    with pytest.raises(ValueError, match="MWW_G_BWD_PAIRS"):
        gts._parse_tables(text.replace("X(30, 24) X(10, 10)", "X(30, 24) Y(10, 10)"))
    with pytest.raises(ValueError, match="fields"):
        gts._parse_tables(text.replace("X(30, 24) X(10, 10)", "X(30, 24, 1) X(10, 10)"))
    slim = gts._parse_tables(text)   # the MWW_SLIM branches are not what is read
    assert slim["MWW_G_WIDTHS"] != (48,) and slim["MWW_G_BWD_PAIRS"] != ((48, 48),)


def test_graph_table_sweep_covers_every_reachable_item():
    """uncovered() is exactly UNREACHABLE: the plan launches every instantiation a flag set can reach and meets every axis item.
    An instantiation deleted from a table (a fused pair, a twin width) leaves the inventory while the plan's route still predicts
    it: case_kernels() must stay inside the inventory."""
    gap = gts.uncovered()
    assert set(gap) == set(gts.UNREACHABLE), ("not covered: %s; listed but covered: %s"
                                               % (sorted(set(gap) - set(gts.UNREACHABLE), key=str), sorted(set(gts.UNREACHABLE) - set(gap), key=str)))
    assert all(isinstance(why, str) and why for why in gts.UNREACHABLE.values())
    inv = gts.inventory()
    planned = set()
    for c in gts.plan():
        ks = set(gts.case_kernels(c))
        assert not ks - inv, (gts.describe(c), ks - inv)
        planned |= ks
    # the fused pairs and twin widths the plan was reviewed with are still instantiated, and launched
    pinned = gts.pinned_instantiations()
    assert not pinned - inv, "gone from graph_launch.hip.h (the engine now falls back without a word): %s" % sorted(pinned - inv)
    assert not pinned - planned - set(gts.UNREACHABLE), sorted(pinned - planned - set(gts.UNREACHABLE))
    t = gts.tables()
    assert set(gts.PINNED_PAIRS) == set(t["pairs"]) and set(gts.PINNED_TWINS) == set(t["twins"]), "update PINNED_* with the header"


def test_graph_table_sweep_notices_a_deleted_instantiation(tmp_path):
    """A table entry deleted from graph_launch.hip.h turns the coverage red: the plan made for the full tables routes through
    the instantiation, the reduced tables' restated rules no longer do, and their inventory no longer holds it."""
    text = open(gts.LAUNCH_H).read()
    for old, new, gone in (("X(48, 32) X(48, 48)", "X(48, 48)", "gconv_bwd_kernel<48, 32>"),
                           ("X(16) X(20) X(24) X(32)\n", "X(16) X(24) X(32)\n", "gconv_bwd2_kernel<20, 20>")):
        assert old in text
        path = tmp_path / ("%d.h" % len(gone))
        path.write_text(text.replace(old, new))
        reduced = gts.tables(str(path))
        assert gone in gts.inventory() and gone not in gts.inventory(reduced)
        planned = {k for c in gts.plan() for k in gts.case_kernels(c)}
        assert gone in planned and gone not in gts.inventory(reduced)
        rerouted = {k for c in gts.plan() for k in gts.case_kernels(c, reduced)}
        assert gone not in rerouted


def test_graph_table_sweep_plan_is_stable(emu_lib):
    """Deterministic, unique ids, inside the issue's shape limits, and the same whichever library is loaded (the plan reads the
    header and the oracle, no library)."""
    cases = gts.plan()
    gts._plan.cache_clear()
    again = gts.plan()
    assert again == cases
    assert len({c["id"] for c in cases}) == len(cases)
    native.NativeLib.get()   # (the product library, next to the emulated one: neither changes the plan)
    assert gts.plan() == cases
    for c in cases:
        assert 40 <= c["T"] <= 212 and c["B"] <= 9, gts.describe(c)
        assert gts._well_posed(c), gts.describe(c)
        if c["kind"] == "mixednet":
            assert len(ec.mo.parse(c["flags"]["pointwise_filters"])) <= 3


def test_graph_table_sweep_has_no_near_zero_unit():
    """No MixedNet case of the plan takes check_graph_mixednet's looser gradient bound (a unit within float32 rounding of a
    ReLU zero, a tie in the attention gate): the count, from the oracle alone, is 0 for every one."""
    for c in gts.plan():
        if c["kind"] == "mixednet":
            assert gts.near_zero_count(c) == 0, gts.describe(c)


SLICE = gts.emulator_slice()


def test_graph_table_sweep_slice_holds_every_launcher():
    want = {gts.launcher_of(k) for k in gts.inventory() - set(gts.UNREACHABLE)}
    got = {gts.launcher_of(k) for c in SLICE for k in gts.case_items(c) if isinstance(k, str)}
    assert got == want, (want - got, got - want)


@pytest.mark.parametrize("case", SLICE, ids=[c["id"] for c in SLICE])
def test_graph_table_sweep_slice(emu_lib, case):
    """A slice of the GPU sweep on the emulated kernels (LDS starts as NaN, buffers end at a guard page): every launcher
    template at least once, against the oracle, with the route check."""
    gts.run_case(emu_lib, case, strict=True)
