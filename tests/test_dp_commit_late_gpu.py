"""Engine option "dp_commit_late" on the GPU (kernels_bwdw.hip.h bwd_blockw_kernel / bwd_firstw_kernel, bwd_first_body.inc): both
orders of the dp commit give the same bits - gradients, parameters after Adam, BN state, probabilities, loss - on the smallest
shapes where moving the commit and its request can go wrong; the float64-oracle bounds hold at the library's default order."""
import pytest

import dp_commit_late_checks as dc
import engine_checks as ec

from microwakeword_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()   # raises loudly if libmww_hip.so is missing
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


B, GRID = 5, 2   # one workgroup owns three windows, the other two: every prefetch crosses a window boundary


@pytest.mark.parametrize("T", [60, 120, 194, 160])
def test_late_commit_is_bit_identical_on_the_default_topology(lib, T):
    """T = 60: one tile per window in every block; 120: two; 194: three with a short last tile; 160: block 4 has Tin = 134 and
    Tout = 114, so its third tile has input rows and no dp rows (group B empty, group A not)."""
    dc.check_late_equals_early(lib, ec.DEF, B, T, GRID)


def test_late_commit_is_bit_identical_with_two_tap_groups_and_relaned_fragments(lib):
    dc.check_late_equals_early(lib, dc.K17_19, B, 194, GRID)


def test_late_commit_is_bit_identical_on_the_notebook_topology(lib):
    """the stride-3 wide first block (tail rows) and the 64-wide blocks"""
    dc.check_late_equals_early(lib, ec.NOTEBOOK, B, 204, GRID)


@pytest.mark.parametrize("x6", [0, 1])
def test_late_commit_is_bit_identical_with_either_conv1_gradient_form(lib, x6):
    """x6 = 1: the g0 planes live in the dp tile's space until the tile's last barrier; x6 = 0 has only the early order"""
    dc.check_late_equals_early(lib, dict(ec.DEF, conv1_x6=x6), B, 194, GRID)


def test_late_commit_is_bit_identical_in_the_wide_x6_first_block(lib):
    dc.check_late_equals_early(lib, dict(ec.DEF, conv1_x6=1, bwd_first_wide=1), B, 194, GRID)


def test_late_commit_is_deterministic(lib):
    a = dc.train_arrays(lib, ec.DEF, B, 194, 1, GRID)
    b = dc.train_arrays(lib, ec.DEF, B, 194, 1, GRID)
    dc.assert_same_bits(a, b, "two runs")


@pytest.mark.parametrize("topology", ["default", "k17_19", "notebook"])
def test_default_order_keeps_the_oracle_bounds(lib, topology):
    flags, T = {"default": (ec.DEF, 194), "k17_19": (dc.K17_19, 194), "notebook": (ec.NOTEBOOK, 204)}[topology]
    ec.check_train_steps(lib, B=B, T=T, steps=2, grid=GRID, flags=flags)
