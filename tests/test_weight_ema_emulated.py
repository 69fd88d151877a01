"""Weight averaging (csrc/kernels_ema.hip.h, ``mww_set_weight_ema`` and the ``ema_forward`` option of the context core,
averaging.py, the ``weight_averaging`` option of the train loop) under the host-side emulator of tests/hipemu; the bodies are in
tests/weight_ema_checks.py."""
import pytest

import weight_ema_checks as we


@pytest.mark.parametrize("kind", we.KINDS)
@pytest.mark.parametrize("every,split", [(1, False), (2, False), (1, True), (2, True)], ids=["every1", "every2", "apply_gradients", "apply_gradients_every2"])
def test_the_average_is_the_restatement_byte_for_byte(emu_lib, kind, every, split):
    we.check_restatement(emu_lib, kind, every, split)


def test_a_non_finite_master_propagates(emu_lib):
    we.check_non_finite_propagates(emu_lib)


@pytest.mark.parametrize("kind", we.KINDS)
def test_the_average_only_observes(emu_lib, kind):
    we.check_observing_only(emu_lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
def test_ema_forward_is_a_twin_whose_master_is_the_average(emu_lib, kind):
    we.check_ema_forward(emu_lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
def test_with_weight_qat_the_shadow_follows_its_source(emu_lib, kind):
    we.check_with_weight_qat(emu_lib, kind)


@pytest.mark.parametrize("kind", ["block", "graph"])
def test_graph_replay_equals_the_eager_run(emu_lib, kind):
    we.check_graph_replay(emu_lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
@pytest.mark.parametrize("every", [1, 2])
def test_state_round_trip_continues_the_same_average(emu_lib, kind, every):
    we.check_state_round_trip(emu_lib, kind, every)


@pytest.mark.parametrize("kind", we.KINDS)
def test_refusals_leave_the_context_usable(emu_lib, kind):
    we.check_refusals(emu_lib, kind)


def test_train_loop_stands_on_the_average_and_restores(emu_lib, tmp_path, caplog, monkeypatch):
    we.check_loop(emu_lib, tmp_path, caplog, monkeypatch)


def test_train_loop_without_the_key_is_unchanged(emu_lib, tmp_path):
    we.check_loop_without_the_key(emu_lib, tmp_path)
