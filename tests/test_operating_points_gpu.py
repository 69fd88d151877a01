"""mww_stream_operating_points (csrc/tu_stream_oppoints.hip) on the MI355X; the bodies (and the shapes: the same as under the
emulator) are in tests/operating_point_checks.py."""
import pytest

import engine_checks as ec
import operating_point_checks as oc
import streaming_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.fixture(scope="module")
def sm(lib):
    _, model = sc.make_model(lib, ec.DEF, 52)
    return sc.streaming.StreamingModel(model, 1, "stream")


@pytest.mark.parametrize("case", list(oc.CASES))
def test_grid_rows_are_the_metrics_and_the_restatement_exactly(sm, case):
    oc.check_grid(sm, case)


def test_operating_point_arguments_are_validated(sm):
    oc.check_validation(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_grid_on_the_kernels_own_probabilities(lib, mode):
    oc.check_own_probabilities(lib, mode)


def test_grid_on_int8_probabilities(lib):
    oc.check_own_probabilities_q8(lib)
