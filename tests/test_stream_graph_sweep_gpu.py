"""Every case of tests/stream_graph_sweep.py on the MI355X: the float graph streaming kernel, its REC (calibration) form and
the int8 graph kernel over every axis Graph::plan accepts, each call held to the float64 / integer oracles - outputs, logits
and rings -, chunking invariance and reruns bit for bit, the non-stream twin.  With MWW_SWEEP_RESULTS=<file> every case
appends its figures (seconds, the largest float logit / probability / ring error and the largest REC range error as shares
of their bounds, the float32 condition, the requantization branches the oracle took) to that file:
profiles/stream_graph_sweep_results.txt holds such a run."""
import json
import os

import pytest

import stream_graph_sweep as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("cid", sw.case_ids())
def test_stream_graph_sweep_case(lib, cid):
    c = sw.case(cid)
    try:
        sw.check_geometry(lib, c)
        res = sw.run_case(lib, c, n_cu=256)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (sw.describe(c), e)) from e
    print("[stream_graph_sweep] %s" % json.dumps(res), flush=True)
    path = os.environ.get("MWW_SWEEP_RESULTS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(res) + "\n")
