"""mww_stream_detections (csrc/tu_stream_detect.hip), detection clips and their closed loop under the host-side emulator of
tests/hipemu; the bodies are in tests/stream_detect_checks.py."""
import pytest

import engine_checks as ec
import stream_detect_checks as dc
import streaming_checks as sc


@pytest.fixture(scope="module")
def sm(emu_lib):
    _, model = sc.make_model(emu_lib, ec.DEF, 52)
    return sc.streaming.StreamingModel(model, 1, "stream")


def test_detections_match_the_restatement_exactly(sm):
    dc.check_against_restatement(sm)


def test_detection_arguments_are_validated(sm):
    dc.check_validation(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_detections_on_the_kernels_own_probabilities(emu_lib, mode):
    dc.check_own_probabilities(emu_lib, mode)


def test_detections_on_int8_probabilities(emu_lib):
    dc.check_own_probabilities_q8(emu_lib)


def test_clips_are_the_windows_that_fired(emu_lib):
    dc.check_clips_closed_loop(emu_lib)
