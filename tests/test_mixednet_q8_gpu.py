"""int8 streaming evaluation of MixedNets with residual connections or a pooled head on the MI355X
(stream_q8_kernel<true> of csrc/tu_stream_q8.hip): every case of tests/quant_mixednet_checks.py - calibration on the device against the old
creator's run and the float64 oracle, resident u16 / f32 tracks, host calls, one-output chains against the literal ring form,
tile edges and the grid-stride loop, the three placements of the tile (LDS below and above 64 KB, global scratch), chunked
calls, reruns and the non_stream twin: uint8 outputs, int8 logits and int8 rings bit for bit against the NumPy restatement."""
import json

import pytest

import quant_mixednet_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("cid", mc.case_ids())
def test_case_equals_the_oracle_bit_for_bit(lib, cid):
    res = mc.run_case(lib, cid, n_cu=256)
    print("[mixednet_q8] %s" % json.dumps(res), flush=True)


def test_abi(lib):
    mc.check_abi(lib)
