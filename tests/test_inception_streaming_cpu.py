"""Conditions on the yardstick of the streaming Inception tests (no kernel runs here): the float64 restatement of
tests/inception_streaming_oracle.py agrees with itself (step form == whole-sequence form), is tied to the graph oracle that is
pinned to the reference (from output T - 1 on it is the non-streaming model on the window ending at the same frame), and
every case the kernel tests use satisfies the input condition (the float32 mode stays within a quarter of each bound)."""
import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_checks as ic
import inception_streaming_oracle as io

TOPOLOGIES = [("INC", ec.INC, 60), ("INC_VARIANT", ec.INC_VARIANT, 60)] + [("random_%d" % i, ec.random_inception_flags(i), 70) for i in range(5)]


def _frames(rng, n):
    return rng.integers(0, 1200, size=(n, 40)).astype(np.float32) * np.float32(0.0390625)


@pytest.mark.parametrize("name,flags,T", TOPOLOGIES, ids=[t[0] for t in TOPOLOGIES])
def test_step_form_equals_whole_sequence_form(name, flags, T):
    om = ec.perturbed_inception_oracle(T, flags)
    net = io.Net(flags, om)
    assert net.reach() == T - 1
    x = _frames(np.random.default_rng(1), T + 40)
    st = io.StepStream(net)
    for n in (0, 1, 7, T + 40):   # the state after n frames, for n below and above every ring length
        z, rings = io.whole_sequence(net, x[:n], rings=True)
        st.reset()
        zs = st.run(x[:n])
        assert rings.size == net.n_state() and zs.shape == z.shape
        assert np.abs(st.state() - rings).max() <= 1e-9
        if n:
            assert np.abs(zs - z).max() <= 1e-9
    # fed in two pieces, the step form carries its state
    st.reset()
    assert np.abs(np.concatenate([st.run(x[:13]), st.run(x[13:])]) - z).max() <= 1e-9


@pytest.mark.parametrize("name,flags,T", TOPOLOGIES, ids=[t[0] for t in TOPOLOGIES])
def test_warm_stream_is_the_non_streaming_model(name, flags, T):
    om = ec.perturbed_inception_oracle(T, flags)
    net = io.Net(flags, om)
    x = _frames(np.random.default_rng(2), T + 25)
    z = io.whole_sequence(net, x)
    ref = io.non_stream_windows(om, x, T, chunk=7)
    assert ref.shape == (26,)
    assert np.abs(z[T - 1:] - ref).max() <= 1e-9
    assert np.abs(z[:T - 1] - ref[0]).max() > 1e-3   # cold rings are a different function of the input


def _condition(net64, net32, frames, what, skip=0):
    z64, r64 = io.whole_sequence(net64, frames, rings=True)
    z32, r32 = io.whole_sequence(net32, frames, rings=True)
    z64, z32 = z64[skip:], z32[skip:]
    if not z64.size:
        return
    ez = np.abs(z32.astype(np.float64) - z64).max()
    ep = np.abs(io.sigmoid(z32).astype(np.float32).astype(np.float64) - io.sigmoid(z64)).max()
    er = np.abs(r32.astype(np.float64) - r64).max() if r64.size else 0.0
    print("%s: float32 restatement uses %.3f of FWD_TOL (logits), %.3f of PROB_TOL, %.3f of FWD_TOL (rings)"
          % (what, ez / ec.FWD_TOL, ep / ic.PROB_TOL, er / ec.FWD_TOL))
    assert ez <= ic.CONDITION * ec.FWD_TOL, (what, ez)
    assert ep <= ic.CONDITION * ic.PROB_TOL, (what, ep)
    assert er <= ic.CONDITION * ec.FWD_TOL, (what, er)


@pytest.mark.parametrize("name", sorted(ic.stream_cases()))
def test_input_condition_of_the_stream_cases(name):
    flags, T, calls, seed = ic.stream_cases()[name]
    om = ec.perturbed_inception_oracle(T, flags)
    frames = ic.all_frames([ic.Tracks(lengths, pads, seed=seed + ci) for ci, (lengths, pads) in enumerate(calls)])
    _condition(io.Net(flags, om), io.Net(flags, om, np.float32), frames, name)


@pytest.mark.parametrize("name", sorted(ic.non_stream_cases()))
def test_input_condition_of_the_non_stream_cases(name):
    flags, T, lengths, pads, seed = ic.non_stream_cases()[name]
    om = ec.perturbed_inception_oracle(T, flags)
    n64, n32 = io.Net(flags, om), io.Net(flags, om, np.float32)
    for t, f in enumerate(ic.Tracks(lengths, pads, seed=seed).frames):
        if len(f) >= T:   # the windows of a track are the warm outputs of the stream fed that track alone
            _condition(n64, n32, f, "%s track %d" % (name, t), skip=T - 1)
