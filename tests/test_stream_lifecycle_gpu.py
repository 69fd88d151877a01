"""The int8 life of a stream - parameters set twice, reset, calibration after quantization - on a MixedNet and a conv/BN
graph stream on the MI355X (tests/stream_lifecycle_checks.py)."""
import pytest

import stream_lifecycle_checks as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("kind", lc.KINDS)
def test_second_parameter_set_equals_a_fresh_stream(lib, kind):
    lc.check_second_parameter_set_equals_a_fresh_stream(lib, kind)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_calibration_after_set_quantized_runs_the_float_kernel(lib, kind):
    lc.check_calibration_after_set_quantized_runs_the_float_kernel(lib, kind)
