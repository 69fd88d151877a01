"""mww_stream_operating_points (csrc/tu_stream_oppoints.hip) and the selection of an operating point under the host-side
emulator of tests/hipemu; the bodies are in tests/operating_point_checks.py."""
import pytest

import engine_checks as ec
import operating_point_checks as oc
import streaming_checks as sc


@pytest.fixture(scope="module")
def sm(emu_lib):
    _, model = sc.make_model(emu_lib, ec.DEF, 52)
    return sc.streaming.StreamingModel(model, 1, "stream")


@pytest.mark.parametrize("case", list(oc.CASES))
def test_grid_rows_are_the_metrics_and_the_restatement_exactly(sm, case):
    oc.check_grid(sm, case)


def test_operating_point_arguments_are_validated(sm):
    oc.check_validation(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_grid_on_the_kernels_own_probabilities(emu_lib, mode):
    oc.check_own_probabilities(emu_lib, mode)


def test_grid_on_int8_probabilities(emu_lib):
    oc.check_own_probabilities_q8(emu_lib)


def test_selection_rule(sm):
    oc.check_selection_rule()
