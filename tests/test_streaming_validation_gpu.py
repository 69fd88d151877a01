"""The streaming_validation option of the train loop (streaming.validate_streaming, train.train) on the MI355X: one run of a few steps at a small batch; the bodies are in
tests/streaming_validation_checks.py."""
import pytest

import streaming_validation_checks as svc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


def test_logged_metrics_are_the_restatement_at_every_boundary(lib, tmp_path):
    svc.check_restatement(lib, tmp_path)
