"""CPU-side checks of the window-descriptor sweep (tests/data_sweep.py): the plan's coverage and stability, the limits it mirrors
against the sources, that its observability check does notice a case that cannot show an error, and the plan itself - minus the
cases marked gpu_only - on the emulated kernels."""
import numpy as np
import pytest

import block_table_sweep as bts
import data_sweep as ds


def test_data_sweep_covers_every_item():
    assert ds.uncovered() == []
    req = set(ds.required())
    kinds = {i[0] for i in req}
    for c in ds.plan():   # (a case may hold more than is required - another B under a grid, say - but nothing of an unknown kind)
        items = ds.case_items(c)
        assert items & req and {i[0] for i in items} <= kinds, (c["id"], items - req)


def test_data_sweep_emulated_subset_covers_everything_but_the_large_stores():
    assert ds.uncovered(ds.emulated_plan()) == [("large-store",)]
    assert [c["id"] for c in ds.plan() if c["gpu_only"]] == [c["id"] for c in ds.plan() if c["kind"] == "large"]


def test_data_sweep_constants_match_the_sources():
    """A changed limit turns the plan red, not stale."""
    got = ds.header_constants()
    assert got == dict(K_XMAX_SAMPLES=ds.K_XMAX_SAMPLES, K_XROW_WORDS=ds.K_XROW_WORDS, K_XMAX_MASKS=ds.K_XMAX_MASKS, K_MAX_MASKS=ds.K_MAX_MASKS,
                       K_GXROWS=ds.K_GXROWS, MAX_STORES=ds.MAX_STORES, SPLIT_RANGE=ds.SPLIT_RANGE)
    import graph_table_sweep as gs
    from microwakeword_amd import native
    assert (gs.K_GXROWS, gs.K_XMAX_SAMPLES, native.MWW_MAX_STORES, native.MAX_MASKS) == (ds.K_GXROWS, ds.K_XMAX_SAMPLES, ds.MAX_STORES, ds.K_MAX_MASKS)


def test_data_sweep_models_are_what_the_plan_assumes(emu_lib):
    """FIRST restates the first blocks of engine_checks.DEF / NOTEBOOK; the strided one is a row of block_table_sweep's table; T_MIN is
    the smallest window DEF takes."""
    import engine_checks as ec
    from microwakeword_amd.layout import MixedNetLayout
    for name, flags in (("DEF", ec.DEF), ("STRIDED", ec.NOTEBOOK)):
        a = MixedNetLayout(flags, 194).engine_args(1)
        assert (a["conv1_kernel"], a["conv1_filters"], a["block_filters"][0], a["block_kernel"][0], a["conv1_stride"]) == ds.FIRST[name]
    assert bts._first_covered(emu_lib, *ds.FIRST["STRIDED"], False) and ds.FIRST["STRIDED"][4] > 1
    MixedNetLayout(ec.DEF, ds.T_MIN)
    with pytest.raises(Exception, match="too short"):
        MixedNetLayout(ec.DEF, ds.T_MIN - 1)


def test_data_sweep_plan_is_stable_and_small():
    cases = ds.plan()
    ds._plan.cache_clear()
    assert ds.plan() == cases
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        assert len(c["windows"]) <= 2 * ds.K_XMAX_SAMPLES + 1 and c["T"] <= ds.T_BITMAP + 1, ds.describe(c)
        if c["kind"] == "route":
            assert c["route"] == ds.expected_route(c), ds.describe(c)
            # every store value of a model-route case is finite and nonzero
            for a in ds.build_stores(c).values():
                assert np.isfinite(a.astype(np.float64)).all() and (a != 0).all() and a.max() <= (666 if a.dtype == np.uint16 else 26), c["id"]


def test_data_sweep_observability_notices_a_blind_case():
    """A window over a store of one repeated row cannot show a wrong src_elem: the check says so."""
    c = next(c for c in ds.plan() if c["id"] == "wg-B2")
    stores = ds.build_stores(c)
    ref = ds.reference_batch(c, stores)
    assert ds.check_observability(c, stores, ref) > 0
    flat = {k: np.tile(a[:ds.BINS], a.size // ds.BINS) for k, a in stores.items()}
    with pytest.raises(AssertionError, match="cannot show a wrong src_elem"):
        ds.check_observability(c, flat, ds.reference_batch(c, flat))
    # ... while a neighbour that names the same cells is no error to show: the width of a mask that already runs past T
    c = next(c for c in ds.plan() if c["id"] == "masks-1-0-T194")
    names = [n for n, *_ in ds.neighbours(c, ds.build_stores(c), 3)]
    assert "tmask0.width+1" in names and ("past-T" in {i[1] for i in ds.case_items(c) if i[0] == "tmask"})
    w, (tm, fm) = c["windows"][3], ds.window_masks(c, 3)
    wider = [(tm[0][0], tm[0][1] + 1)]
    assert np.array_equal(ds.symbolic(w, tm, fm, c["T"]), ds.symbolic(w, wider, fm, c["T"]))


PLAN = ds.emulated_plan()


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_data_sweep_emulated(emu_lib, case):
    ds.run_case(emu_lib, case)
