"""Hard-negative mining and the zero-copy mined training provider under the host-side emulator of tests/hipemu; the bodies are
in tests/mining_checks.py."""
import mining_checks as mc


def test_mining_and_the_mined_provider_non_stream(emu_lib):
    mc.check_mining_and_mined_provider(emu_lib, "non_stream")


def test_mining_and_the_mined_provider_stream(emu_lib):
    mc.check_mining_and_mined_provider(emu_lib, "stream")


def test_a_running_prefetcher_is_rebuilt(emu_lib):
    mc.check_prefetcher_is_rebuilt(emu_lib)


def test_sharded_handlers_and_foreign_clips_are_refused(emu_lib):
    mc.check_refusals(emu_lib)


def test_mining_a_testing_set_warns(emu_lib, caplog):
    mc.check_testing_mode_warns(emu_lib, caplog)
