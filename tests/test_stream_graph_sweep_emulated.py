"""CPU side of the graph streaming sweep (tests/stream_graph_sweep.py): the plan covers every required item but the written-down
unreachable ones, the restated geometry of Graph::plan agrees with every number the library exposes, the three conditions
on every case's inputs (oracles only, no kernel), the description-driven float oracle pinned to the Inception one, the limits
Graph::plan refuses at, and an ``emulator_slice()`` of the plan through the kernels under the host-side emulator of
tests/hipemu (its fibers run a block's threads one after the other up to each barrier: a missing barrier is a
deterministic mismatch)."""
import ctypes as C

import numpy as np
import pytest

import engine_checks as ec
import inception_streaming_oracle as io
import quant_graph_checks as qgc
import stream_graph_oracle as sgo
import stream_graph_sweep as sw
import streaming_checks as sc

REQUIRED_BY_THE_ISSUE = 91   # items of required(): a plan that silently drops one fails here


def test_plan_covers_every_required_item():
    assert len(sw.required()) == len(set(sw.required())) == REQUIRED_BY_THE_ISSUE
    assert sw.uncovered() == list(sw.UNREACHABLE) and all(len(why) > 40 for why in sw.UNREACHABLE.values())
    # a plan without a case leaves exactly that case's own items uncovered: uncovered() is not vacuous
    rest = [c for c in sw.cases() if c.id != "arena_plans-differ"]
    assert {"arena:plans-reuse-differently", "arena:flags-differ"} <= set(sw.uncovered(rest))
    rest = [c for c in sw.cases() if c.id != "sources_slices_diamond_unread"]
    assert {"src:n=3", "src:same-tensor-twice", "src:three-consumers", "dag:unread-middle", "ring:three-unequal-sources",
            "src:slice-ends-at-unpadded-row-end"} <= set(sw.uncovered(rest))
    assert sum(not c.spread for c in sw.cases()) <= 1


def test_restated_plan_of_the_hand_made_cases():
    """the figures the cases' comments state, from the restatement: the int8 tiles on either side of 160 KB, the two plans
    that part, the barrier no written source asks for"""
    pl = {c.id: sw.plan_of(c.id) for c in sw.cases()}
    assert pl["lds-largest_w592"].tile_bytes == 163688 <= sw.KMAX_LDS == 163840 < pl["scratch-smallest_w596"].tile_bytes == 164724
    assert 64 * 1024 < pl["lds-mid_w300"].tile_bytes == 10360 + 259 * 300 <= sw.KMAX_LDS
    p = pl["arena_plans-differ"]
    assert p.f32.sync == [1, 1, 0, 1] and p.q8.sync == [1, 1, 1, 1]
    assert p.f32.buf[2] != p.f32.buf[0] and p.q8.buf[2] == p.q8.buf[0] and p.q8.why[2] == (True, False, False)
    p = pl["arena_late-input_out-read-only"]
    assert p.in_last == 2 and p.f32.buf[2] == p.f32.buf[0] and p.f32.why[2] == (True, False, False) and p.f32.sync[4] == 0
    p = pl["sources_slices_diamond_unread"]
    assert p.last_use[4] == -1 and p.reach[4] == 0 and p.reach[0] == p.reach[2] + p.R[2] > p.reach[5] and p.R[6] * p.cin[6] == 2 * 23
    assert pl["k1-only"].n_state == 3 * 2 and pl["d1024_k2_tf1"].n_state == 1024 * 2
    assert pl["chain48"].n == 48 and pl["w1024_final-map-2^18"].tf * 1024 == 1 << 18


@pytest.mark.parametrize("cid", sw.case_ids())
def test_restated_geometry_equals_the_library(emu_lib, cid):
    sw.check_geometry(emu_lib, sw.case(cid))


@pytest.mark.parametrize("cid", sw.case_ids())
def test_case_inputs_meet_the_conditions(cid):
    """oracles only: the float32 restatement within CONDITION of every bound of the float64 one; spread-out int8 logits;
    every source of a multi-source op and every tap of a k > 1 op on a path to the head moves a float64 logit by more than
    twice FWD_TOL and changes an int8 logit.  (A "nospread" case has constant int8 logits by construction - a hand-set range
    puts a ReLU output's zero point at 127 - so only the float half of the sensitivity is asked of it.)"""
    c = sw.case(cid)
    f = sw.float32_condition(cid)
    print("[stream_graph_sweep] %s float32 restatement / bound: logits %.4f probabilities %.4f rings %.4f" % ((cid,) + f))
    assert max(f) <= sw.CONDITION, (sw.describe(c), f)
    b = sw.built(cid)
    if c.spread:
        print("[stream_graph_sweep] %s spread %s" % (cid, qgc.check_spread(b.qm, b.seq, cid)))
    sens = sw.sensitivity(cid)
    if sens:
        print("[stream_graph_sweep] %s sensitivity over %d sources / taps: smallest float64 logit change %.3g, fewest int8 logits changed %d"
              % (cid, len(sens), min(s[1] for s in sens), min(s[2] for s in sens)))
    for what, df, nq in sens:
        assert df > 2 * ec.FWD_TOL, (cid, what, df)
        assert nq > 0 or not c.spread, (cid, what, "no int8 logit changes")
    assert b.net.n_state() == sw.plan_of(cid).n_state


@pytest.mark.parametrize("name", ["INC", "INC_VARIANT", "RANDOM_3", "RANDOM_7"])
def test_oracle_equals_the_inception_oracle(name):
    """the description-driven oracle on an Inception description (streaming.graph_stream_description) against the
    flags-driven one: logits, rings and the non-stream windows to 1e-11"""
    from microwakeword_amd import streaming
    flags = {"INC": ec.INC, "INC_VARIANT": ec.INC_VARIANT}.get(name) or ec.random_inception_flags(int(name.split("_")[1]))
    T = 60
    om = ec.perturbed_inception_oracle(T, flags, seed=42)
    desc = streaming.graph_stream_description(flags, T, 1, "stream")
    net, ref = sgo.Net(desc, om.get_weights()), io.Net(flags, om)
    assert (net.tf, net.c_last, net.n_state()) == (ref.tf, ref.c_last, ref.n_state())
    x = sw.gen_frames(np.random.default_rng(5), 150, "u16")
    z, st = sgo.whole_sequence(net, x, rings=True)
    rz, rst = io.whole_sequence(ref, x, rings=True)
    assert np.abs(z - rz).max() <= 1e-11 and np.abs(st - rst).max() <= 1e-11, (np.abs(z - rz).max(), np.abs(st - rst).max())
    w = sgo.non_stream_windows(net, x[:T + 9], T)
    rw = io.non_stream_windows(om, x[:T + 9], T)
    assert w.shape == rw.shape == (10,) and np.abs(w - rw).max() <= 1e-11
    assert np.abs(w - z[T - 1:T + 9]).max() <= 1e-9   # past the warm-up no ring is read: both forms see the same frames


@pytest.mark.parametrize("cid", ["sources_slices_diamond_unread", "arena_late-input_out-read-only", "d1024_k2_tf1", "k1-only", "chain48"])
def test_step_oracle_equals_whole_sequence_oracle(cid):
    b = sw.built(cid)
    x = b.seq[:40] if cid != "d1024_k2_tf1" else b.seq[:1100]
    step = sgo.StepStream(b.net)
    z, st = sgo.whole_sequence(b.net, x, rings=True)
    assert np.abs(step.run(x) - z).max() < 1e-9 and np.abs(step.state() - st).max() < 1e-9, cid
    assert step.state().size == b.net.n_state()


def test_emulator_slice(emu_lib):
    import time
    t0 = time.time()
    for c in sw.emulator_slice():
        try:
            res = sw.run_case(emu_lib, c, n_cu=4)   # the emulated device has 4 CUs
        except AssertionError as e:
            raise AssertionError("%s\n%s" % (sw.describe(c), e)) from e
        print("[stream_graph_sweep] emulated %s" % res, flush=True)
    print("[stream_graph_sweep] emulator slice: %d cases in %.0f s" % (len(sw.emulator_slice()), time.time() - t0))


# ------------------------------------------------------------------------------------------------------ refusals
def _create(model, desc, tweak=None, int8=False):
    """mww_stream_create_convnet[_q8] on ``desc`` with the C description edited by ``tweak`` (what native.GraphStream does,
    without its own argument checks: n_ops = 49 and n_src = 4 reach the library)"""
    from microwakeword_amd import native
    nl = model.engine.nl
    d = native.ConvNetDesc()
    d.frames, d.dropout, d.max_batch = int(desc["frames"]), 0.0, 1
    native._fill_conv_ops(d, list(desc["conv_ops"]))
    if tweak:
        tweak(d)
    h = C.c_void_p()
    create = nl.lib.mww_stream_create_convnet_q8 if int8 else nl.lib.mww_stream_create_convnet
    nl.check(create(model.engine.h, C.byref(d), native.STREAM_MODES[desc.get("mode", "stream")], C.byref(h)))
    assert h.value
    nl.lib.mww_stream_destroy(h)


def _refused(model, desc, message, tweak=None):
    from microwakeword_amd import native
    if tweak is None:   # the restated planner answers the same refusal
        assert sw.Plan(desc).refusal is not None and message.replace("\\", "") in "error -3: " + sw.Plan(desc).refusal, (message, sw.Plan(desc).refusal)
    for int8 in (False, True):
        with pytest.raises(native.NativeError, match=message):
            _create(model, desc, tweak, int8)


def _accepted(model, desc, tweak=None):
    assert sw.Plan(desc).refusal is None
    _create(model, desc, tweak)
    _create(model, desc, tweak, int8=True)


def _with(desc, i, frames=None, **fields):
    ops = [dict(o) for o in desc["conv_ops"]]
    ops[i].update(fields)
    return dict(desc, conv_ops=ops, frames=desc["frames"] if frames is None else frames)


def test_plan_refuses_at_its_limits_and_accepts_just_inside(emu_lib):
    """every ``bad(...)`` line of Graph::plan that a description can reach, with its message, and the value next to it"""
    model = sc.context_model(emu_lib)
    U = "error -3: "
    op = sw.op
    base = sw.desc_of([op([-1], k=3, f=6, g=2), op([0], k=2, d=2, f=4), op([0, 1, -1], f=5, sl=[(2, 3), (0, 0), (36, 4)])], 2)   # window 6
    _accepted(model, base)
    # n_ops
    _refused(model, dict(base, conv_ops=[]), U + r"n_ops must be 1\.\.48")
    chain = sw.case("chain48").desc
    _accepted(model, chain)

    def forty_nine(d):
        d.n_ops = 49
    _refused(model, chain, U + r"n_ops must be 1\.\.48", forty_nine)
    # frames, and a window one frame too short for the graph
    _refused(model, dict(base, frames=0), U + "frames must be positive")
    _refused(model, dict(base, frames=-3), U + "frames must be positive")
    short = sw.desc_of([op([-1], k=3, f=6), op([0], k=2, d=2, f=4)], 1)   # window 5, drops all zero
    _accepted(model, short)
    _refused(model, dict(short, frames=4), U + r"op 1: kernel does not fit frames = 4 \(the window is too short for this graph\)")
    _refused(model, dict(short, frames=2), U + r"op 0: kernel does not fit frames = 2 \(the window is too short for this graph\)")
    # src: an earlier op or -1
    _refused(model, _with(base, 1, src=[1]), U + "op 1: src must name an earlier op or -1")
    _refused(model, _with(base, 1, src=[2]), U + "op 1: src must name an earlier op or -1")
    _refused(model, _with(base, 0, src=[0]), U + "op 0: src must name an earlier op or -1")
    _refused(model, _with(base, 1, src=[-2]), U + "op 1: src must name an earlier op or -1")
    # src_drop: leaves a frame, aligns the sources (base: op 2 reads op 0 (4 frames, drop 2), op 1 (2 frames), the input (6, drop 4))
    assert base["conv_ops"][2]["drop"] == [2, 0, 4]
    _refused(model, _with(base, 2, drop=[2, 2, 4]), U + "op 2: src_drop must leave at least one frame")
    _refused(model, _with(base, 2, drop=[2, -1, 4]), U + "op 2: src_drop must leave at least one frame")
    _refused(model, _with(base, 0, drop=[6]), U + "op 0: src_drop must leave at least one frame")
    _accepted(model, _with(base, 2, drop=[3, 1, 5]))   # one frame each
    _refused(model, _with(base, 2, drop=[2, 0, 3]), U + "op 2: src_drop does not align the sources to one length")
    _refused(model, _with(base, 2, drop=[1, 0, 4]), U + "op 2: src_drop does not align the sources to one length")
    # slices
    S = U + "op 2: src_c0 / src_cn is not a slice of the source"
    _refused(model, _with(base, 2, slice=[(2, 5), (0, 0), (36, 4)]), S)      # 2 + 5 > 6 channels
    _refused(model, _with(base, 2, slice=[(2, 3), (0, 0), (36, 5)]), S)      # 36 + 5 > 40 bins
    _refused(model, _with(base, 2, slice=[(6, 0), (0, 0), (36, 4)]), S)      # the whole rest of nothing
    _refused(model, _with(base, 2, slice=[(-1, 3), (0, 0), (36, 4)]), S)
    _refused(model, _with(base, 2, slice=[(2, -1), (0, 0), (36, 4)]), S)
    _accepted(model, _with(base, 2, slice=[(2, 4), (3, 1), (39, 1)]))
    # kernel, dilation, filters at 0 and 1025, accepted at 1 and 1024
    for field in ("kernel", "dilation", "filters"):
        for v in (0, 1025, -1):
            _refused(model, _with(base, 0, **{field: v}), U + r"op 0: %s must be 1\.\.1024" % field)
    one = sw.desc_of([op([-1], f=2, sl=[(7, 1)])], 1)
    _accepted(model, one)
    _accepted(model, _with(one, 0, frames=1024, kernel=1024))
    _refused(model, _with(one, 0, frames=1023, kernel=1024), U + r"op 0: kernel does not fit frames = 1023")
    _accepted(model, _with(one, 0, frames=1025, kernel=2, dilation=1024))
    _accepted(model, _with(one, 0, dilation=1024))   # k = 1: the dilation reaches nothing
    _accepted(model, _with(one, 0, filters=1024, bn_groups=1024))
    # bn_groups
    G = U + "op 0: bn_groups must divide the filters"
    _refused(model, _with(base, 0, bn_groups=4), G)
    _refused(model, _with(base, 0, bn_groups=0), G)
    _refused(model, _with(base, 0, bn_groups=12), G)
    _accepted(model, _with(base, 0, bn_groups=6))
    _accepted(model, _with(base, 0, bn_groups=3))
    # n_src
    _refused(model, _with(base, 1, src=[], drop=[], slice=[]), U + r"op 1: n_src must be 1\.\.3")

    def four_sources(d):
        d.ops[2].n_src = 4
    _refused(model, base, U + r"op 2: n_src must be 1\.\.3", four_sources)
    # the final map against the head's 2^24 values
    wide = sw.desc_of([op([-1], f=1024, sl=[(0, 1)])], 1 << 14)
    _accepted(model, wide)
    _refused(model, dict(wide, frames=wide["frames"] + 1), U + "frames leaves a final map too large for the head")
    # what the vocabulary leaves out
    _refused(model, dict(base, mode="stream"), U + "head_pool is outside the streaming graph vocabulary", lambda d: setattr(d, "head_pool", 1))
    _refused(model, base, U + "op 1: residual is outside the streaming graph vocabulary", lambda d: setattr(d.ops[1], "residual", 1))


def test_a_stream_works_after_a_refusal(emu_lib):
    from microwakeword_amd import native
    model = sc.context_model(emu_lib)
    b = sw.built("arena_plans-differ")
    st = native.GraphStream(model.engine, b.desc)
    st.set_weights(b.flat)
    st.run_host(b.seq[:50])
    with pytest.raises(native.NativeError, match="kernel must be"):
        native.GraphStream(model.engine, _with(b.desc, 0, kernel=0))
    with pytest.raises(native.NativeError, match="src must name"):
        native.GraphStream(model.engine, _with(b.desc, 1, src=[3]), int8=True)
    st.run_host(b.seq[50:120])
    p, z = st.read(want_logits=True)
    ref, ref_st = sgo.whole_sequence(b.net, b.seq[:120], rings=True)
    sc._compare(p, z, ref[50:], "after a refusal")
    sw.compare_state(st.get_state(), ref_st, b.net, "after a refusal")
    st.close()
