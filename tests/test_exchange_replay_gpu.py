"""W > 1 data-parallel steps on the MI355X, one process, one device: every case of tests/exchange_checks.py through the replay
rendezvous of tests/exchange_replay.py (no process group, no child process, no graph capture).  What the world-1 RCCL tests of
tests/test_engine_gpu.py cannot see - 1 / W in the statistics, the gradient scale and Adam's step, which range of the gradient
goes to the hook and when, the partial-row and single-launch routes sync-BN switches to - is held here to the float64 oracle on
the global batch at the bounds of the W = 1 checks.  What it does not show: the overlap of a deferred bucket with the backward
kernels, and RCCL itself."""
import pytest

import exchange_checks as xc
from microwakeword_amd import native

pytestmark = pytest.mark.gpu

# the cases are read from the library's own shape table (host-only: collection needs the built library, not a GPU)
BLOCK_CASES = xc.block_cases(native.NativeLib.get())
GRAPH_CASES = xc.graph_cases()


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c["id"] for c in BLOCK_CASES])
def test_sync_bn_block_engine(lib, case):
    xc.report(case["id"], xc.check_sync_bn_block(lib, case))


@pytest.mark.parametrize("case", GRAPH_CASES, ids=[c["id"] for c in GRAPH_CASES])
def test_sync_bn_graph_engine(lib, case):
    xc.report(case["id"], xc.check_sync_bn_graph(lib, case))


@pytest.mark.parametrize("kind", ["mixednet", "inception"])
def test_throughput_mode_is_a_composition_of_single_device_pieces(lib, kind):
    xc.report("throughput-" + kind, xc.check_throughput_composition(lib, kind))


def test_weight_qat_behind_the_exchange(lib):
    xc.report("weight-qat", xc.check_weight_qat(lib))


def test_weight_ema_behind_the_exchange(lib):
    xc.report("weight-ema", xc.check_weight_ema(lib))


def test_bn_reestimation_with_sync_bn(lib):
    xc.report("bn-reestimate-sync-bn", xc.check_bn_reestimate_sync(lib))
