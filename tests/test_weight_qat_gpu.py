"""Weight-only quantization-aware training on the MI355X; the bodies (and the shapes: the same as under the emulator) are in
tests/weight_qat_checks.py."""
import pytest

import weight_qat_checks as wq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("kind", wq.KINDS)
def test_shadow_is_the_restatement_bit_for_bit(lib, kind):
    wq.check_shadow_bits(lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_train_step_is_the_oracle_step_at_the_shadow(lib, kind, monkeypatch):
    wq.check_train_steps_at_the_shadow(lib, kind, monkeypatch)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_inference_reads_the_shadow(lib, kind):
    wq.check_inference(lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_off_is_off(lib, kind):
    wq.check_off_is_off(lib, kind)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_toggling_mid_run(lib, kind, monkeypatch):
    wq.check_toggle_mid_run(lib, kind, monkeypatch)


def test_graph_replay_equals_the_eager_run(lib):
    wq.check_graph_replay(lib)


@pytest.mark.parametrize("kind", wq.KINDS)
def test_refusals_leave_the_context_usable(lib, kind):
    wq.check_refusals(lib, kind)


def test_train_loop_turns_the_option_on_and_restores(lib, tmp_path, caplog):
    wq.check_loop(lib, tmp_path, caplog)


def test_train_loop_without_the_key_is_unchanged(lib, tmp_path):
    wq.check_loop_without_the_key(lib, tmp_path)
