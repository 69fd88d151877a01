"""Un-waited call sequences across the ring of eight mailboxes against the same calls made one at a time, bit for bit
(tests/pipeline_checks.py), on an MI355X: the event wait of mail_begin, the hyper words read at execution time, labels read in
place from a mailbox's HBM copy, descriptor-only batches and the cache of captured steps under the load the train loop and
mww_evaluate_windows put on them."""
import pytest

import pipeline_checks as pc
from microwakeword_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()  # raises loudly if libmww_hip.so is missing
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("graphs", [0, 1])
def test_learning_rate_per_step_over_three_laps(lib, graphs, depth):
    pc.check_lr_ring(lib, "mixednet", T=60, B=8, steps=26, graphs=graphs, depth=depth)


def test_adam_slots_against_float64_restatement(lib):
    pc.check_adam_restatement(lib, T=60, B=8, steps=26)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind,T", [("mixednet", 60), ("notebook", 204)])
def test_mixed_call_scripts(lib, kind, T, seed):
    unwaited = pc.check_mixed_script(lib, seed, kind, T=T, Bmax=8, graphs=seed % 2)
    print("most commits without a host wait: %d" % unwaited)


@pytest.mark.parametrize("graphs", [0, 1])
def test_a_slot_met_again_by_a_captured_step(lib, graphs):
    pc.check_mixed_script(lib, "revisit", "mixednet", T=60, Bmax=8, graphs=graphs)


def test_evaluation_across_the_ring(lib):
    pc.check_evaluation_ring(lib, "mixednet", T=60, batch=4, full=19, rest=3)


@pytest.mark.parametrize("graphs", [0, 1])
@pytest.mark.parametrize("kind,T", [("inception", 100), ("inception", 212), ("graph_mixednet", 100)])
def test_graph_engine_learning_rate_per_step(lib, kind, T, graphs):
    pc.check_lr_ring(lib, kind, T=T, B=8, steps=20, graphs=graphs, depth=0)


@pytest.mark.parametrize("graphs", [0, 1])
@pytest.mark.parametrize("kind,T", [("mixednet", 60), ("graph_mixednet", 60)])
def test_training_state_is_complete(lib, kind, T, graphs):
    pc.check_training_state_is_complete(lib, kind, T=T, B=8, N=9, graphs=graphs)
