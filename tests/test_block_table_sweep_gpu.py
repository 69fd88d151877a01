"""Every instantiation of the specialised block kernels against the float64 oracle: one train step per case of the covering plan
of tests/block_table_sweep.py (every (shape, form) of csrc/block_launch.hip.h's table at least once, every strided first block
in tail mode and over two tiles).  A case's id names the instantiation it was built around, e.g. ``b48x64k21-last-narrow-fp32``
(block 48 -> 64 channels, 21-tap depthwise, LAST form of the 256-thread backward kernel, fp32 mode)."""
import pytest

import block_table_sweep as bts
import engine_checks as ec
from microwakeword_amd import mixednet, native

pytestmark = pytest.mark.gpu

# the plan is read from the library's own shape table (host-only: collection needs the built library, not a GPU)
PLAN = bts.plan(native.NativeLib.get())


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_block_table_sweep(lib, case):
    flags = bts.case_flags(case)
    assert mixednet.kernel_family(flags, case["T"], lib=lib, bf16=case["mode"] > 0)[0] == "block", bts.describe(case)
    try:
        ec.check_train_steps(lib, B=case["B"], T=case["T"], steps=1, grid=case["grid"], flags=flags)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (bts.describe(case), e)) from None
