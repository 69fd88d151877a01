"""BatchNorm re-estimation for the weight average (csrc/kernels_bnre.hip.h, ``mww_bn_reestimate_*``, averaging.py, the
``weight_averaging.bn_reestimate`` option of the train loop) under the host-side emulator of tests/hipemu; the bodies are in
tests/bn_reestimate_checks.py."""
import pytest

import bn_reestimate_checks as bc

KIND_INLINE = [(k, i) for k in bc.KINDS for i in bc.INLINE]
IDS = ["%s-%s" % (k, "inline" if i else "finalize") for k, i in KIND_INLINE]


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_passes_compose_byte_for_byte(emu_lib, kind, inline):
    bc.check_composition(emu_lib, kind, inline)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_the_statistics_are_the_forwards_own_byte_for_byte(emu_lib, kind, inline):
    bc.check_forwards_own_statistics(emu_lib, kind, inline)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_against_the_float64_oracle(emu_lib, kind, inline):
    bc.check_against_oracle(emu_lib, kind, inline)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_evaluation_is_a_twin_with_the_reestimated_statistics(emu_lib, kind, inline):
    bc.check_evaluation_is_a_twin(emu_lib, kind, inline)


@pytest.mark.parametrize("graphs", [0, 1], ids=["eager", "graphs"])
@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_a_pass_only_observes(emu_lib, kind, inline, graphs):
    bc.check_observing_only(emu_lib, kind, inline, graphs)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_invalidation_returns_to_the_masters_statistics(emu_lib, kind, inline):
    bc.check_invalidation(emu_lib, kind, inline)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_with_weight_qat_the_pass_reads_the_shadow_of_the_average(emu_lib, kind, inline):
    bc.check_with_weight_qat(emu_lib, kind, inline)


@pytest.mark.parametrize("kind,inline", KIND_INLINE, ids=IDS)
def test_the_windows_form_is_the_three_calls(emu_lib, kind, inline):
    bc.check_windows_form(emu_lib, kind, inline)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_refusals_leave_the_context_usable(emu_lib, kind):
    bc.check_refusals(emu_lib, kind)


def test_train_loop_writes_and_validates_on_the_reestimated_statistics(emu_lib, tmp_path, caplog, monkeypatch):
    bc.check_loop(emu_lib, tmp_path, caplog, monkeypatch)


def test_train_loop_without_the_key_keeps_the_masters_statistics(emu_lib, tmp_path, monkeypatch):
    bc.check_loop_without_the_key(emu_lib, tmp_path, monkeypatch)


def test_bad_settings_are_refused_before_step_0(emu_lib, tmp_path):
    bc.check_bad_settings(emu_lib, tmp_path)
