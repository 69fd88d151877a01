"""mww_set_option's table on a MixedNet and a conv/BN graph context under the host-side emulator of tests/hipemu
(tests/option_table_checks.py)."""
import pytest

import option_table_checks as oc


@pytest.mark.parametrize("kind", oc.KINDS)
def test_documented_names_at_their_defaults(emu_lib, kind):
    oc.check_documented_names_at_their_defaults(emu_lib, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_ranges_and_unknown_names(emu_lib, kind):
    oc.check_ranges_and_unknown_names(emu_lib, kind)


def test_bf16_is_refused_on_a_graph_context(emu_lib):
    oc.check_bf16_is_refused_on_a_graph_context(emu_lib)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_options_of_the_other_engine_change_nothing(emu_lib, kind):
    oc.check_options_of_the_other_engine_change_nothing(emu_lib, kind)


def test_replay_is_separated_by_an_option_change(emu_lib):
    oc.check_replay_is_separated_by_an_option_change(emu_lib)
