"""Hard-negative mining and the zero-copy mined training provider on the MI355X; the bodies are in tests/mining_checks.py."""
import pytest

import mining_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from microwakeword_amd import native
    nl = native.NativeLib.get()
    if nl.device_count() < 1:
        pytest.fail("no GPU visible")
    return nl


def test_mining_and_the_mined_provider_non_stream(lib):
    mc.check_mining_and_mined_provider(lib, "non_stream")


def test_mining_and_the_mined_provider_stream(lib):
    mc.check_mining_and_mined_provider(lib, "stream")


def test_a_running_prefetcher_is_rebuilt(lib):
    mc.check_prefetcher_is_rebuilt(lib)


def test_sharded_handlers_and_foreign_clips_are_refused(lib):
    mc.check_refusals(lib)


def test_mining_a_testing_set_warns(lib, caplog):
    mc.check_testing_mode_warns(lib, caplog)
