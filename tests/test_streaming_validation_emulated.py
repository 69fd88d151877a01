"""The streaming_validation option of the train loop (streaming.validate_streaming, train.train) under the host-side emulator of tests/hipemu; the bodies are in
tests/streaming_validation_checks.py."""
import streaming_validation_checks as svc


def test_logged_metrics_are_the_restatement_at_every_boundary(emu_lib, tmp_path):
    svc.check_restatement(emu_lib, tmp_path)


def test_the_key_alone_changes_nothing_in_training(emu_lib, tmp_path):
    svc.check_unnamed_changes_nothing(emu_lib, tmp_path)


def test_best_weights_follow_the_streaming_metrics(emu_lib, tmp_path):
    svc.check_selection_follows_streaming(emu_lib, tmp_path)


def test_no_window_meets_the_target(emu_lib, tmp_path):
    svc.check_no_window_meets_the_target(emu_lib, tmp_path)


def test_refusals_come_before_the_first_step(emu_lib, tmp_path, monkeypatch):
    svc.check_refusals(emu_lib, tmp_path, monkeypatch)


def test_streaming_validation_with_hard_negative_mining(emu_lib, tmp_path):
    svc.check_with_mining(emu_lib, tmp_path)


def test_a_validation_draws_nothing(emu_lib):
    svc.check_draws_nothing(emu_lib)
