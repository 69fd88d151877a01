"""Streaming evaluation of MixedNets with residual connections, a pooled head or spatial attention on the MI355X
(stream_forward_kernel<true, *> of csrc/tu_stream.hip): every case of tests/mixednet_variant_checks.py - resident u16 / f32 tracks with pads and empty
tracks, host calls, one-output chains against the literal ring form, tile edges and the grid-stride loop, the non_stream twin,
outputs, logits and rings against the float64 oracles, chunked predict_spectrogram and reruns bit for bit -, the
reference-graph fixture and the refusals of the ABI."""
import json

import pytest

import mixednet_variant_checks as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("cid", vc.case_ids())
def test_case_matches_the_oracles(lib, cid):
    res = vc.run_case(lib, vc.case(cid), n_cu=256)
    print("[mixednet_variant] %s" % json.dumps(res), flush=True)


def test_reference_graph_fixture(lib, golden_dir):
    vc.check_reference_fixture(lib, golden_dir)


def test_abi_refusals(lib):
    vc.check_abi_refusals(lib)
