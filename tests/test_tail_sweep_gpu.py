"""The kernels every train step ends in - head_kernel, the dense-weight gradient, the metric update, gradient assembly and Adam -
against tests/tail_oracle.py, the float64 restatement fed with the engine's own head inputs, at derived bounds: one case of the
covering plan of tests/tail_sweep.py per test.  A case's id names its anchor: ``head48x12-upper-grid1`` (head_kernel<48, 12> at
T_final = 21 x 12 under "grid_head" 1, B = 3), ``dense-T8-B1025-routeA`` (grad_final's dense role on the 32 x 8 model: the first
batch past the pair path), ``metrics-p0.5-clipped``, ``graph-res-rdrop-B288``."""
import pytest

import tail_sweep as ts
from microwakeword_amd import native

pytestmark = pytest.mark.gpu

# the plan is read from mww_lib.hip and the oracle alone: collection needs no GPU
PLAN = ts.plan()


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_tail_sweep(lib, case):
    ts.run_case(lib, case)
