"""The bootstrap sub-mapping of streaming_validation in the train loop under the host-side emulator of tests/hipemu; the bodies are
in tests/operating_bootstrap_loop_checks.py."""
import operating_bootstrap_loop_checks as blc


def test_bounds_are_logged_restated_and_selected_on(emu_lib, tmp_path):
    blc.check_loop(emu_lib, tmp_path)


def test_without_the_sub_mapping_nothing_changes(emu_lib, tmp_path, caplog):
    blc.check_without_the_sub_mapping(emu_lib, tmp_path, caplog)


def test_a_validation_with_the_bootstrap_draws_nothing(emu_lib):
    blc.check_draws_nothing(emu_lib)


def test_bootstrap_settings_are_refused_before_the_first_step(emu_lib, tmp_path, monkeypatch):
    blc.check_refusals(emu_lib, tmp_path, monkeypatch)
