"""mww_stream_calibrate (csrc/tu_stream_calibrate.hip) and the quantized streaming validation of the train loop on the MI355X;
the bodies (and the shapes: the same as under the emulator) are in tests/int8_in_loop_checks.py."""
import pytest

import int8_in_loop_checks as ilc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("name", ilc.KERNEL_CASES)
def test_calibrate_equals_the_host_form_and_the_float_run(lib, name):
    ilc.check_calibrate(lib, name)


def test_calibrate_refusals(lib):
    ilc.check_calibrate_refusals(lib)


def test_quantized_validation_logs_the_restatement(lib, tmp_path, caplog):
    ilc.check_restatement(lib, tmp_path, caplog)
