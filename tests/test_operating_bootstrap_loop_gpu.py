"""The bootstrap sub-mapping of streaming_validation in the train loop on the MI355X: one run of a few steps at a small batch; the
body is in tests/operating_bootstrap_loop_checks.py."""
import pytest

import operating_bootstrap_loop_checks as blc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


def test_bounds_are_logged_restated_and_selected_on(lib, tmp_path):
    blc.check_loop(lib, tmp_path, rerun=False)
