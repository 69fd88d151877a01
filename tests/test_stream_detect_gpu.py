"""mww_stream_detections (csrc/tu_stream_detect.hip), detection clips and their closed loop on the MI355X; the bodies (and
the shapes: the same as under the emulator) are in tests/stream_detect_checks.py."""
import pytest

import engine_checks as ec
import stream_detect_checks as dc
import streaming_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


@pytest.fixture(scope="module")
def sm(lib):
    _, model = sc.make_model(lib, ec.DEF, 52)
    return sc.streaming.StreamingModel(model, 1, "stream")


def test_detections_match_the_restatement_exactly(sm):
    dc.check_against_restatement(sm)


def test_detection_arguments_are_validated(sm):
    dc.check_validation(sm)


@pytest.mark.parametrize("mode", ["stream", "non_stream"])
def test_detections_on_the_kernels_own_probabilities(lib, mode):
    dc.check_own_probabilities(lib, mode)


def test_detections_on_int8_probabilities(lib):
    dc.check_own_probabilities_q8(lib)


def test_clips_are_the_windows_that_fired(lib):
    dc.check_clips_closed_loop(lib)
