"""Sharpness-aware train steps and global-norm gradient clipping on the MI355X; the bodies (and the shapes: the same as under
the emulator) are in tests/sharpness_checks.py."""
import pytest

import sharpness_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("lazy", [False, True], ids=["x", "descriptors"])
def test_a_sharpness_aware_step_is_its_twin_byte_for_byte(lib, kind, lazy):
    sc.check_twin(lib, kind, lazy=lazy)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clipped", "below_the_threshold"])
def test_a_sharpness_aware_step_with_clipping_is_its_twin(lib, kind, factor):
    sc.check_twin(lib, kind, clip_factor=factor)


def test_masked_taps_do_not_move(lib):
    sc.check_masked_taps_do_not_move(lib)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_final_gradient_is_the_float64_oracle_s_at_the_perturbed_point(lib, kind):
    sc.check_oracle_at_the_perturbed_point(lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("graphs", [0, 1], ids=["eager", "graphs"])
def test_installing_and_removing_only_observes(lib, kind, graphs):
    sc.check_observing_only(lib, kind, graphs)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_clipping_is_the_restatement_and_exact_below_the_threshold(lib, kind):
    sc.check_clipping(lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_with_weight_qat_the_second_pass_reads_the_shadow_of_the_perturbed_master(lib, kind):
    sc.check_twin(lib, kind, weight_qat=True)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_weight_average_takes_one_update_per_step_behind_the_restore(lib, kind):
    sc.check_with_weight_average(lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_under_graphs_the_step_has_the_bytes_of_the_eager_step(lib, kind):
    sc.check_graphs_option(lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_a_non_finite_gradient_propagates(lib, kind):
    sc.check_non_finite(lib, kind)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_refusals_leave_the_context_as_it_was(lib, kind):
    sc.check_refusals(lib, kind)


def test_train_loop_with_both_options(lib, tmp_path, caplog):
    sc.check_loop(lib, tmp_path, caplog)


def test_train_loop_without_the_keys_is_unchanged(lib, tmp_path):
    sc.check_loop_without_the_keys(lib, tmp_path)
