"""mww_stream_mine (csrc/tu_stream_mine.hip), mining on the device, FeatureHandler.set_mined_clips and the hard_negative_mining
option of the train loop under the host-side emulator of tests/hipemu; the bodies are in tests/stream_mine_checks.py."""
import pytest

import stream_mine_checks as smc


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
@pytest.mark.parametrize("stride", [1, 3])
def test_kernel_equals_the_host_chain(emu_lib, stride, mode):
    smc.check_kernel(emu_lib, stride, mode)


def test_kernel_validation(emu_lib):
    smc.check_kernel_validation(emu_lib)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_mining_on_device_equals_mining_on_the_host(emu_lib, mode):
    smc.check_through_model(emu_lib, mode)


def test_mining_on_device_on_an_int8_stream(emu_lib):
    smc.check_through_model(emu_lib, "stream", quantized=True)


def test_set_mined_clips_refusals_and_replacement(emu_lib):
    smc.check_set_mined_clips_refusals(emu_lib)


def test_set_mined_clips_at_weight_zero_with_a_running_prefetcher(emu_lib):
    smc.check_set_mined_clips_weight_zero(emu_lib)


def test_loop_mines_at_the_boundaries(emu_lib, tmp_path):
    smc.check_loop_rounds(emu_lib, tmp_path)


def test_loop_without_detections(emu_lib, tmp_path):
    smc.check_loop_no_detections(emu_lib, tmp_path)


def test_loop_merge_rule_and_restore(emu_lib, tmp_path):
    smc.check_loop_merge_and_restore(emu_lib, tmp_path)


def test_loop_refusals(emu_lib, tmp_path, monkeypatch):
    smc.check_loop_refusals(emu_lib, tmp_path, monkeypatch)
