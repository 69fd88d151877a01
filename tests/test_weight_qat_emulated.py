"""Weight-only quantization-aware training (csrc/kernels_qat.hip.h, the ``weight_qat`` option of the context core, qat.py, the
``weight_quantization_aware`` option of the train loop) under the host-side emulator of tests/hipemu; the bodies are in
tests/weight_qat_checks.py."""
import pytest

import weight_qat_checks as wq


@pytest.mark.parametrize("kind", wq.KINDS)
def test_shadow_is_the_restatement_bit_for_bit(emu_lib, kind):
    wq.check_shadow_bits(emu_lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_train_step_is_the_oracle_step_at_the_shadow(emu_lib, kind, monkeypatch):
    wq.check_train_steps_at_the_shadow(emu_lib, kind, monkeypatch)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_inference_reads_the_shadow(emu_lib, kind):
    wq.check_inference(emu_lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_off_is_off(emu_lib, kind):
    wq.check_off_is_off(emu_lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_toggling_mid_run(emu_lib, kind, monkeypatch):
    wq.check_toggle_mid_run(emu_lib, kind, monkeypatch)


def test_graph_replay_equals_the_eager_run(emu_lib):
    wq.check_graph_replay(emu_lib)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_refusals_leave_the_context_usable(emu_lib, kind):
    wq.check_refusals(emu_lib, kind)


def test_train_loop_turns_the_option_on_and_restores(emu_lib, tmp_path, caplog):
    wq.check_loop(emu_lib, tmp_path, caplog)


def test_train_loop_without_the_key_is_unchanged(emu_lib, tmp_path):
    wq.check_loop_without_the_key(emu_lib, tmp_path)


def test_train_loop_refusals_come_before_any_file(emu_lib, tmp_path):
    wq.check_loop_refusals(emu_lib, tmp_path)
