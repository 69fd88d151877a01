"""Sharpness-aware train steps and global-norm gradient clipping (csrc/kernels_sam.hip.h, ``mww_set_sharpness_aware`` /
``mww_set_grad_clip`` of the context core, sharpness.py, the ``sharpness_aware`` / ``gradient_clipping`` options of the train
loop) under the host-side emulator of tests/hipemu; the bodies are in tests/sharpness_checks.py."""
import pytest

import sharpness_checks as sc


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("lazy", [False, True], ids=["x", "descriptors"])
def test_a_sharpness_aware_step_is_its_twin_byte_for_byte(emu_lib, kind, lazy):
    sc.check_twin(emu_lib, kind, lazy=lazy)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clipped", "below_the_threshold"])
def test_a_sharpness_aware_step_with_clipping_is_its_twin(emu_lib, kind, factor):
    sc.check_twin(emu_lib, kind, clip_factor=factor)


def test_masked_taps_do_not_move(emu_lib):
    sc.check_masked_taps_do_not_move(emu_lib)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_final_gradient_is_the_float64_oracle_s_at_the_perturbed_point(emu_lib, kind):
    sc.check_oracle_at_the_perturbed_point(emu_lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("graphs", [0, 1], ids=["eager", "graphs"])
def test_installing_and_removing_only_observes(emu_lib, kind, graphs):
    sc.check_observing_only(emu_lib, kind, graphs)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_clipping_is_the_restatement_and_exact_below_the_threshold(emu_lib, kind):
    sc.check_clipping(emu_lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_with_weight_qat_the_second_pass_reads_the_shadow_of_the_perturbed_master(emu_lib, kind):
    sc.check_twin(emu_lib, kind, weight_qat=True)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_weight_average_takes_one_update_per_step_behind_the_restore(emu_lib, kind):
    sc.check_with_weight_average(emu_lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_under_graphs_the_step_has_the_bytes_of_the_eager_step(emu_lib, kind):
    sc.check_graphs_option(emu_lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_a_non_finite_gradient_propagates(emu_lib, kind):
    sc.check_non_finite(emu_lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_refusals_leave_the_context_as_it_was(emu_lib, kind):
    sc.check_refusals(emu_lib, kind)


def test_train_loop_with_both_options(emu_lib, tmp_path, caplog):
    sc.check_loop(emu_lib, tmp_path, caplog)


def test_train_loop_without_the_keys_is_unchanged(emu_lib, tmp_path):
    sc.check_loop_without_the_keys(emu_lib, tmp_path)
