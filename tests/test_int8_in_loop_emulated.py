"""mww_stream_calibrate (csrc/tu_stream_calibrate.hip), quantize.calibration_windows / LoopQuantizer and the ``quantized`` key of
the streaming_validation and hard_negative_mining options of the train loop under the host-side emulator of tests/hipemu; the
bodies are in tests/int8_in_loop_checks.py."""
import pytest

import int8_in_loop_checks as ilc


@pytest.mark.parametrize("name", ilc.KERNEL_CASES)
def test_calibrate_equals_the_host_form_and_the_float_run(emu_lib, name):
    ilc.check_calibrate(emu_lib, name)


def test_calibrate_refusals(emu_lib):
    ilc.check_calibrate_refusals(emu_lib)


def test_calibration_windows_are_fixed_and_draw_from_no_shared_generator(emu_lib):
    ilc.check_calibration_windows(emu_lib)


def test_quantized_validation_logs_the_restatement(emu_lib, tmp_path, caplog):
    ilc.check_restatement(emu_lib, tmp_path, caplog)


def test_float_validation_log_line_is_unchanged(emu_lib, tmp_path, caplog):
    ilc.check_float_log_line(emu_lib, tmp_path, caplog)


def test_quantized_keys_without_a_streaming_metric_change_nothing(emu_lib, tmp_path):
    ilc.check_unnamed_changes_nothing(emu_lib, tmp_path)


def test_best_weights_follow_the_int8_metrics(emu_lib, tmp_path):
    ilc.check_selection_follows_int8(emu_lib, tmp_path)


def test_quantized_mining_and_one_calibration_per_boundary(emu_lib, tmp_path, monkeypatch):
    ilc.check_mining_quantized(emu_lib, tmp_path, monkeypatch)


def test_quantized_options_draw_nothing(emu_lib):
    ilc.check_draws_nothing(emu_lib)


def test_quantized_refusals(emu_lib, tmp_path, monkeypatch):
    ilc.check_refusals(emu_lib, tmp_path, monkeypatch)


@pytest.mark.parametrize("family", ["inception", "residual"])
def test_quantized_dry_validation_of_the_other_families(emu_lib, tmp_path, family):
    ilc.check_families(emu_lib, tmp_path, family)
