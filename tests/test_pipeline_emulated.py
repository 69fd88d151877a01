"""Un-waited call sequences against the same calls made one at a time (tests/pipeline_checks.py), under the host-side emulator of
tests/hipemu.  Launches run inline there, so ordering cannot fail; what these runs cover is the host logic of csrc/mww_lib.hip -
which mailbox slot holds a descriptor-only batch, where the labels are, what a captured step is keyed by - which differs between
the twins ("fused_input", "graphs")."""
import pytest

import pipeline_checks as pc


@pytest.mark.parametrize("seed,graphs", [(0, 1), (1, 0)])
def test_mixed_call_scripts(emu_lib, seed, graphs):
    pc.check_mixed_script(emu_lib, seed, "mixednet", T=60, Bmax=4, graphs=graphs)


@pytest.mark.parametrize("graphs", [0, 1])
def test_a_slot_met_again_by_a_captured_step(emu_lib, graphs):
    pc.check_mixed_script(emu_lib, "revisit", "mixednet", T=60, Bmax=4, graphs=graphs)


def test_adam_slots_against_float64_restatement(emu_lib):
    """(the stepwise twin alone: what a pair of twins cannot see, being wrong together)"""
    pc.check_adam_restatement(emu_lib, T=60, B=4, steps=10)


def test_evaluation_across_the_ring(emu_lib):
    pc.check_evaluation_ring(emu_lib, "mixednet", T=60, batch=4)


@pytest.mark.parametrize("graphs", [0, 1])
@pytest.mark.parametrize("kind,T", [("mixednet", 60), ("graph_mixednet", 60)])
def test_training_state_is_complete(emu_lib, kind, T, graphs):
    pc.check_training_state_is_complete(emu_lib, kind, T=T, B=4, N=9, graphs=graphs)
