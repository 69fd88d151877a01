"""The int8 life of a stream - parameters set twice, reset, calibration after quantization - on a MixedNet and a conv/BN
graph stream under the host-side emulator of tests/hipemu (tests/stream_lifecycle_checks.py)."""
import pytest

import stream_lifecycle_checks as lc


@pytest.mark.parametrize("kind", lc.KINDS)
def test_second_parameter_set_equals_a_fresh_stream(emu_lib, kind):
    lc.check_second_parameter_set_equals_a_fresh_stream(emu_lib, kind)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_calibration_after_set_quantized_runs_the_float_kernel(emu_lib, kind):
    lc.check_calibration_after_set_quantized_runs_the_float_kernel(emu_lib, kind)
