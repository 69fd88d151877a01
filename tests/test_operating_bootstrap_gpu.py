"""mww_stream_operating_bootstrap (csrc/tu_stream_bootstrap.hip) on the MI355X; the bodies (and the shapes: the same as under the
emulator) are in tests/operating_bootstrap_checks.py."""
import pytest

import engine_checks as ec
import operating_bootstrap_checks as obc
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
def test_records_are_the_restatement_exactly(sm, case):
    obc.check_grid_cases(sm, case)


def test_blocks_at_the_segment_boundaries_carry_the_cooldown(sm):
    obc.check_block_borders(sm)


@pytest.mark.parametrize("n_pos", [1, obc.P - 1, obc.P, obc.P + 1, 4 * obc.P + 1])
def test_positive_levels_around_the_level_workgroup(sm, n_pos):
    obc.check_positive_counts(sm, n_pos)


def test_comparison_is_strict_and_short_tracks_are_never_accepted(sm):
    obc.check_strict_comparison(sm)


def test_reselection_follows_the_rule_on_the_device(sm):
    obc.check_selection(sm)


def test_identical_units_give_intervals_without_width(sm):
    obc.check_degenerate(sm)


def test_operating_bootstrap_arguments_are_validated(sm):
    obc.check_arguments(sm)


def test_one_kind_only(sm):
    obc.check_one_kind(sm)


def test_interleaved_calls_share_buffers_without_a_trace(sm):
    obc.check_shared_buffers(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_bootstrap_on_the_kernels_own_probabilities(lib, mode):
    obc.check_own_probabilities(lib, mode)


def test_bootstrap_on_int8_probabilities(lib):
    obc.check_own_probabilities_q8(lib)
