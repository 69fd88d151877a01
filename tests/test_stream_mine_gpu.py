"""mww_stream_mine (csrc/tu_stream_mine.hip), mining on the device, FeatureHandler.set_mined_clips and the hard_negative_mining
option of the train loop on the MI355X; the bodies (and the shapes: the same as under the emulator) are in
tests/stream_mine_checks.py."""
import pytest

import stream_mine_checks as smc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
@pytest.mark.parametrize("stride", [1, 3])
def test_kernel_equals_the_host_chain(lib, stride, mode):
    smc.check_kernel(lib, stride, mode)


def test_kernel_validation(lib):
    smc.check_kernel_validation(lib)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_mining_on_device_equals_mining_on_the_host(lib, mode):
    smc.check_through_model(lib, mode)


def test_mining_on_device_on_an_int8_stream(lib):
    smc.check_through_model(lib, "stream", quantized=True)


def test_set_mined_clips_refusals_and_replacement(lib):
    smc.check_set_mined_clips_refusals(lib)


def test_set_mined_clips_at_weight_zero_with_a_running_prefetcher(lib):
    smc.check_set_mined_clips_weight_zero(lib)


def test_loop_mines_at_the_boundaries(lib, tmp_path):
    smc.check_loop_rounds(lib, tmp_path)


def test_loop_without_detections(lib, tmp_path):
    smc.check_loop_no_detections(lib, tmp_path)


def test_loop_merge_rule_and_restore(lib, tmp_path):
    smc.check_loop_merge_and_restore(lib, tmp_path)


def test_loop_refusals(lib, tmp_path, monkeypatch):
    smc.check_loop_refusals(lib, tmp_path, monkeypatch)
