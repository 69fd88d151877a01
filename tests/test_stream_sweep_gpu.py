"""Every case of tests/stream_sweep.py on the MI355X: the float streaming kernel, its REC (calibration) form and the int8
kernel over every topology axis plan() accepts, each call held to the float64 / integer oracles - outputs, logits and
rings -, chunking invariance and reruns bit for bit, stream against non_stream mode.  With MWW_SWEEP_RESULTS=<file> every
case appends its figures (seconds, largest float logit / ring error and their share of FWD_TOL, requantization branches
the oracle took) to that file: profiles/stream_sweep_results.txt is such a run."""
import json
import os

import pytest

import stream_sweep as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("cid", sw.case_ids())
def test_stream_sweep_case(lib, cid):
    c = sw.case(cid)
    try:
        res = sw.run_case(lib, c, n_cu=256)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (sw.describe(c), e)) from e
    print("[stream_sweep] %s" % json.dumps(res), flush=True)
    path = os.environ.get("MWW_SWEEP_RESULTS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(res) + "\n")
