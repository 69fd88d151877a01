"""Every reader of window descriptors - the assembly kernel, the "fused_input" gather of the first block's kernels, the gathering
stem of the conv/BN graph engine, the window-list calls, the streaming kernels and the mined clips - at the edges of the
descriptors and of the SpecAugment masks, bit for bit: one case of the covering plan of tests/data_sweep.py per test.  A case's id
names its anchor: ``desc-edges`` (copy_rows 0 / 1 / T - 1 / T, windows ending on their store's last element),
``masks-8-0-T194`` (eight time masks per window, the gather's limit, at the bitmap's word edges), ``wg-B17-fwd4-bwd2-materialised``
(the forward grid would let the first block gather, the backward grid does not), ``large-stores`` (windows across element 2^31 and
byte 2^32 of their store)."""
import pytest

import data_sweep as ds
from microwakeword_amd import native

pytestmark = pytest.mark.gpu

# the plan is built from the module's constants alone: collection needs no GPU
PLAN = ds.plan()


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("case", PLAN, ids=[c["id"] for c in PLAN])
def test_data_sweep(lib, case):
    ds.run_case(lib, case)
