"""mww_set_option's table on a MixedNet and a conv/BN graph context on the MI355X (tests/option_table_checks.py)."""
import pytest

import option_table_checks as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("kind", oc.KINDS)
def test_documented_names_at_their_defaults(lib, kind):
    oc.check_documented_names_at_their_defaults(lib, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_ranges_and_unknown_names(lib, kind):
    oc.check_ranges_and_unknown_names(lib, kind)


def test_bf16_is_refused_on_a_graph_context(lib):
    oc.check_bf16_is_refused_on_a_graph_context(lib)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_options_of_the_other_engine_change_nothing(lib, kind):
    oc.check_options_of_the_other_engine_change_nothing(lib, kind)


def test_replay_is_separated_by_an_option_change(lib):
    oc.check_replay_is_separated_by_an_option_change(lib)
