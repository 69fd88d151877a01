"""mww_stream_operating_summary (csrc/tu_stream_oppoints.hip) under the host-side emulator of tests/hipemu; the bodies are in
tests/operating_summary_checks.py."""
import pytest

import engine_checks as ec
import operating_point_checks as oc
import operating_summary_checks as osc
import streaming_checks as sc


@pytest.fixture(scope="module")
def sm(emu_lib):
    _, model = sc.make_model(emu_lib, ec.DEF, 52)
    return sc.streaming.StreamingModel(model, 1, "stream")


@pytest.mark.parametrize("case", list(oc.CASES))
def test_summary_is_the_grid_reduced_and_the_restatement_exactly(sm, case):
    osc.check_grid_cases(sm, case)


def test_cooldown_walk_at_the_segment_boundaries(sm):
    osc.check_cooldown_boundaries(sm)


@pytest.mark.parametrize("n_pos", [1, osc.P - 1, osc.P, osc.P + 1, 4 * osc.P + 1])
def test_positive_counts_around_the_reduction_workgroup(sm, n_pos):
    osc.check_positive_counts(sm, n_pos)


def test_comparison_is_strict_and_short_tracks_are_never_accepted(sm):
    osc.check_strict_comparison(sm)


def test_one_kind_only(sm):
    osc.check_one_kind(sm)


def test_operating_summary_arguments_are_validated(sm):
    osc.check_validation(sm)


def test_interleaved_calls_share_buffers_without_a_trace(sm):
    osc.check_shared_buffers(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_summary_on_the_kernels_own_probabilities(emu_lib, mode):
    osc.check_own_probabilities(emu_lib, mode)


def test_summary_on_int8_probabilities(emu_lib):
    osc.check_own_probabilities_q8(emu_lib)
