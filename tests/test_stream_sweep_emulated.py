"""CPU side of the streaming sweep (tests/stream_sweep.py): the plan covers every required item, its tile-placement
arithmetic, the two conditions on every case's inputs (oracle only, no kernel), the limits plan() and
mww_stream_set_quantized refuse at, and an ``emulator_slice()`` of the plan (every item once, cheapest cases first) through
the kernels under the host-side emulator of tests/hipemu."""
import numpy as np
import pytest

import q8_checks as qc
import stream_sweep as sw
import streaming_checks as sc

REQUIRED_BY_THE_ISSUE = 83   # items of required(): a plan that silently drops one fails here


def test_plan_covers_every_required_item():
    assert len(sw.required()) == len(set(sw.required())) == REQUIRED_BY_THE_ISSUE
    assert sw.uncovered() == []
    # a plan without a case leaves exactly that case's own items uncovered: uncovered() is not vacuous
    rest = [c for c in sw.cases() if c.id != "w13-9_g3-eq_k1eq-s3_tf1"]
    assert {"conv1:k1==s", "head:tf=1", "mix:equal-neighbours", "mix:K1-first-block"} <= set(sw.uncovered(rest))
    assert len({c.id for c in sw.cases()}) == len(sw.cases())
    assert sum(not c.spread for c in sw.cases()) <= 2


def test_tile_placement_arithmetic():
    """bytes = ((256 + reach1 - 1) * s + k1) * 40 + 2 * (256 + reach1) * r4(cmax) against kMaxLds = 160 KB, restated (the
    library's choice is not observable without a launch): one case below 64 KB, one between, and the two next to the limit"""
    by = {c.id: c for c in sw.cases()}
    assert sw.tile_bytes(by["lds-largest_w288"].desc) == 162704 <= sw.KMAX_LDS == 163840
    assert sw.tile_bytes(by["scratch-smallest_w292"].desc) == 164816 > sw.KMAX_LDS
    assert sw.reach1_of(by["lds-largest_w288"].desc) == sw.reach1_of(by["scratch-smallest_w292"].desc) == 8
    assert 64 * 1024 < sw.tile_bytes(by["lds-mid_w200"].desc) <= sw.KMAX_LDS
    assert sw.tile_bytes(by["one-block_s1"].desc) < 64 * 1024
    assert sw.tile_placement(by["w1024"].desc) == "scratch"


@pytest.mark.parametrize("cid", sw.case_ids())
def test_case_inputs_meet_the_conditions(cid):
    """oracle only: the float32 restatement within a quarter of every bound of the float64 one, and (int8) spread-out logits"""
    c = sw.case(cid)
    f = sw.float32_condition(cid)
    print("[stream_sweep] %s float32 restatement / bound: logits %.3f probabilities %.3f rings %.3f" % ((cid,) + f))
    assert max(f) <= 0.25, (sw.describe(c), f)
    b = sw.built(cid)
    if c.spread:
        print("[stream_sweep] %s spread %s" % (cid, qc.check_spread(b.qm, b.seq, cid)))
    assert sw.reach1_of(c.desc) == b.net.tf - 1 + sum(b.net.ring_sizes()[1:-1])


def test_fixed_synthetic_ranges_fail_the_spread_condition():
    """why synthetic_quantized takes ranges: with its fixed ones an odd topology compares a near-constant"""
    b = sw.built("w30-50-7_g3-rem_k1lt-s3")
    distinct, share, _ = qc.spread(qc.synthetic_quantized(b.desc), b.seq)
    assert distinct < qc.SPREAD_MIN_DISTINCT or share > qc.SPREAD_MAX_SHARE
    qm = qc.synthetic_quantized(b.desc, ranges=b.qm.ranges)
    assert np.array_equal(qm.zero_points, b.qm.zero_points)


def test_step_oracles_equal_whole_sequence_oracles():
    """the two forms of each oracle agree on the odd topologies too (logits and rings)"""
    import quant_oracle as qo
    import streaming_oracle as so
    for cid in ("w30-50-7_g3-rem_k1lt-s3", "w13-9_g3-eq_k1eq-s3_tf1", "s4_k1-last"):
        b = sw.built(cid)
        x = b.seq[:60 * b.s + b.s - 1]
        step = so.StepStream(b.net)
        z, st = so.whole_sequence(b.net, x, rings=True)
        assert np.abs(step.run(x) - z).max() < 1e-9 and np.abs(step.state() - st).max() < 1e-9, cid
        qstep = qo.StepStreamQ8(b.qm)
        u8, _, qst = qo.whole_sequence(b.qm, x)
        assert np.array_equal(qstep.run(x), u8) and np.array_equal(qstep.state(), qst), cid


def test_emulator_slice(emu_lib):
    import time
    t0 = time.time()
    for c in sw.emulator_slice():
        try:
            res = sw.run_case(emu_lib, c, n_cu=4)   # the emulated device has 4 CUs
        except AssertionError as e:
            raise AssertionError("%s\n%s" % (sw.describe(c), e)) from e
        print("[stream_sweep] emulated %s %.1f s, float logit error %.2e ring error %.2e" % (c.id, res["seconds"], res["logit_err"],
                                                                                          res["state_err"]), flush=True)
    print("[stream_sweep] emulator slice: %d cases in %.0f s" % (len(sw.emulator_slice()), time.time() - t0))


BASE = dict(conv1_filters=8, conv1_kernel=3, stride=1, blocks=[(1, (3,), 8), (1, (5,), 4)], t_final=2, frames=10, mode="stream")


def _refused(model, desc, message, exc=None):
    from microwakeword_amd import native
    with pytest.raises(exc or native.NativeError, match=message):
        native.Stream(model.engine, desc)


def _accepted(model, desc):
    from microwakeword_amd import native
    native.Stream(model.engine, desc).close()


def test_plan_refuses_at_its_limits_and_accepts_just_inside(emu_lib):
    model = sc.context_model(emu_lib)
    blk = (1, (3,), 8)
    U = r"error -3: "
    _accepted(model, BASE)
    _refused(model, dict(BASE, blocks=[]), U + r"n_blocks must be 1\.\.8")
    _refused(model, dict(BASE, blocks=[blk] * 9), "at most 8 blocks", NotImplementedError)
    _accepted(model, dict(BASE, blocks=[blk]))
    _accepted(model, dict(BASE, blocks=[blk] * 8))
    _refused(model, dict(BASE, blocks=[(0, (3,), 8)]), U + r"block 0: repeat must be 1\.\.8")
    _refused(model, dict(BASE, blocks=[blk, (9, (3,), 8)]), U + r"block 1: repeat must be 1\.\.8")
    _accepted(model, dict(BASE, blocks=[(8, (3,), 8)]))
    _refused(model, dict(BASE, blocks=[(1, (), 8)]), U + r"block 0: 1\.\.8 MixConv kernels")
    _refused(model, dict(BASE, blocks=[(1, (1, 2, 3, 4, 5, 6, 7, 8, 9), 8)]), "at most 8 MixConv kernels", NotImplementedError)
    _accepted(model, dict(BASE, blocks=[(1, (1, 2, 3, 4, 5, 6, 7, 8), 8)]))
    _refused(model, dict(BASE, conv1_filters=2, blocks=[(1, (3, 5, 7), 8)]), U + "more MixConv groups than channels")
    _accepted(model, dict(BASE, conv1_filters=3, blocks=[(1, (3, 5, 7), 8)]))
    _refused(model, dict(BASE, blocks=[(1, (3,), 0)]), U + r"block 0: pointwise filters must be 1\.\.1024")
    _refused(model, dict(BASE, blocks=[(1, (3,), 1025)]), U + r"block 0: pointwise filters must be 1\.\.1024")
    _accepted(model, dict(BASE, blocks=[(1, (3,), 1)]))
    _accepted(model, dict(BASE, blocks=[(1, (3,), 1024)]))
    _refused(model, dict(BASE, blocks=[(1, (5, 3), 8)]), U + "mixconv kernel sizes must be ascending")
    _accepted(model, dict(BASE, blocks=[(1, (3, 3), 8)]))
    _refused(model, dict(BASE, blocks=[(1, (0, 3), 8)]), U + "block 0: kernel sizes must be positive")
    _refused(model, dict(BASE, t_final=0), U + "t_final must be positive")
    _accepted(model, dict(BASE, t_final=1))
    # non_stream: frames against the first convolution's kernel and t_final against the window
    ns = dict(BASE, mode="non_stream", conv1_kernel=3, blocks=[(1, (1,), 8)], frames=3, t_final=1)
    _accepted(model, ns)
    _refused(model, dict(ns, frames=2), U + "non_stream mode needs frames >= the first convolution's kernel")
    ns = dict(BASE, mode="non_stream")   # 10 frames: 8 after conv1, 8 - 2 - 4 = 2 final frames
    _accepted(model, ns)
    _refused(model, dict(ns, t_final=1), U + r"t_final 1 does not match a 10-frame window \(2 final frames\)")
    _refused(model, dict(ns, t_final=3), U + r"t_final 3 does not match a 10-frame window \(2 final frames\)")


def test_set_quantized_refuses_shifts_and_multipliers_the_device_cannot_take(emu_lib):
    """int32 values come from any .npz: a shift outside [-31, 30] or a negative multiplier would reach x >> e, e >= 32"""
    from microwakeword_amd import native
    model = sc.context_model(emu_lib)
    b = sw.built("rq-shifts")   # carries both edges, -31 and +30: accepted
    w, iv, scale, lut = b.qm.packed()
    st = native.Stream(model.engine, b.desc)
    st.set_quantized(w, iv, scale, lut)
    c1 = b.desc["conv1_filters"]
    n_i = iv.size
    dense_at = n_i - (len(sw.layers_of(b.desc)) + 3) - 3   # the Dense's (bias, multiplier, shift)
    for at, value in ((2 * c1, 31), (2 * c1, -32), (c1, -1), (dense_at + 2, 31), (dense_at + 2, -32), (dense_at + 1, -5),
                      (3 * c1 + 2 * 8 + 1, 31), (3 * c1 + 8 + 1, -(1 << 31))):   # conv1, the Dense, the first MixConv behind conv1
        bad = iv.copy()
        bad[at] = value
        with pytest.raises(native.NativeError, match="error -1: requantization multipliers must be >= 0 and shifts lie in"):
            st.set_quantized(w, bad, scale, lut)
    for at, value in ((2 * c1, 30), (2 * c1, -31), (c1, 0), (dense_at + 2, -31)):
        ok = iv.copy()
        ok[at] = value
        st.set_quantized(w, ok, scale, lut)
    st.close()
