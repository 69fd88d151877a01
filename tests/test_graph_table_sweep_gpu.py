"""Every instantiation of the conv/BN graph training kernels against the float64 oracle: one train step per case of the covering
plan of tests/graph_table_sweep.py (every instantiation of csrc/graph_launch.hip.h's tables that a flag set can reach, and the
grid / frame-chunk / weight-gradient-part / depthwise / BN / static-shape / gathering-stem / head axes), at the bounds of
engine_checks.check_graph_mixednet (its looser gradient bound an assertion failure) and check_inception_train_steps, followed by
the route check: the launch names one more step records under "profile" equal graph_table_sweep.case_route(case).  A case's id
names its anchor, e.g. ``pair48x32-chunk3-grid2`` (fused weight + data gradient of a 32 -> 48 1x1 op, three frame chunks,
"grid_graph" 2 with B = 5), ``pw60x20-split-chunk2-auto``, ``twin20-k5d2-g2-finalize``."""
import pytest

import graph_table_sweep as gts
from microwakeword_amd import native

pytestmark = pytest.mark.gpu

# the plan is read from graph_launch.hip.h and the oracle alone: collection needs no GPU
PLAN = gts.plan()


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_graph_table_sweep(lib, case):
    gts.run_case(lib, case, strict=True)
