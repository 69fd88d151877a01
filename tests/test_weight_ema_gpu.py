"""Weight averaging on the MI355X; the bodies (and the shapes: the same as under the emulator) are in
tests/weight_ema_checks.py."""
import pytest

import weight_ema_checks as we

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("kind", we.KINDS)
@pytest.mark.parametrize("every,split", [(1, False), (2, False), (1, True), (2, True)], ids=["every1", "every2", "apply_gradients", "apply_gradients_every2"])
def test_the_average_is_the_restatement_byte_for_byte(lib, kind, every, split):
    we.check_restatement(lib, kind, every, split)


def test_a_non_finite_master_propagates(lib):
    we.check_non_finite_propagates(lib)


@pytest.mark.parametrize("kind", we.KINDS)
def test_the_average_only_observes(lib, kind):
    we.check_observing_only(lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
def test_ema_forward_is_a_twin_whose_master_is_the_average(lib, kind):
    we.check_ema_forward(lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
def test_with_weight_qat_the_shadow_follows_its_source(lib, kind):
    we.check_with_weight_qat(lib, kind)


@pytest.mark.parametrize("kind", ["block", "graph"])
def test_graph_replay_equals_the_eager_run(lib, kind):
    we.check_graph_replay(lib, kind)


@pytest.mark.parametrize("kind", we.KINDS)
@pytest.mark.parametrize("every", [1, 2])
def test_state_round_trip_continues_the_same_average(lib, kind, every):
    we.check_state_round_trip(lib, kind, every)


@pytest.mark.parametrize("kind", we.KINDS)
def test_refusals_leave_the_context_usable(lib, kind):
    we.check_refusals(lib, kind)


def test_train_loop_stands_on_the_average_and_restores(lib, tmp_path, caplog, monkeypatch):
    we.check_loop(lib, tmp_path, caplog, monkeypatch)


def test_train_loop_without_the_key_is_unchanged(lib, tmp_path):
    we.check_loop_without_the_key(lib, tmp_path)
