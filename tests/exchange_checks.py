"""W > 1 data-parallel steps on one device: the cases of tests/test_exchange_replay_emulated.py (tests/hipemu, a fixed slice)
and tests/test_exchange_replay_gpu.py (every case), run through tests/exchange_replay.py.

(b) sync-BN parity: W ranks of Bl windows against the float64 oracle's single step on the W * Bl windows, through the
    comparison halves of engine_checks (compare_mixednet_step, compare_inception_step, compare_graph_mixednet_step - the code
    path and the bounds of the W = 1 checks), the ranks' reads merged by engine_checks.merge_rank_reads.
(c) throughput mode (rank-local BatchNorm) as a composition of single-device pieces: the reduced gradient is the float32
    rank-order sum of the ranks' STEP_NO_APPLY gradients, the parameters apply_gradients(lr, 1 / W) on that sum - the check
    that sees a dropped 1 / W, which Adam alone is blind to.
(d) step features behind the exchange: weight QAT, the weight average, BN re-estimation with sync-BN on.

Every check returns a record for profiles/exchange_replay_results.txt: exchanges, runs, seconds, worst error-to-bound ratio."""
import time

import numpy as np

import block_table_sweep as bts
import engine_checks as ec
import graph_table_sweep as gts
from exchange_replay import Memory, replay
from microwakeword_amd import native
from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout, MixedNetLayout

LR = 1e-3
IN_ORDER, DEFERRED, FLUSH = native.EXCHANGE_IN_ORDER, native.EXCHANGE_DEFERRED, native.EXCHANGE_FLUSH


def batch(rng, B, T):
    x = ec.synth_x(rng, B, T)
    y = (rng.random(B) < 0.5).astype(np.float32)
    return x, y, rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32)


def _record(t0, ex, ratio, **more):
    return dict(exchanges=len(ex), runs=ex.runs, seconds=time.time() - t0, ratio=float(ratio), **more)


def _step(eng, Bl, r, x, y, w, keep=None, flags=0):
    sl = slice(r * Bl, (r + 1) * Bl)
    eng.set_batch(x[sl])
    eng.set_targets(y[sl], w[sl])
    if keep is not None:
        eng.set_dropout_mask(keep[sl])
    eng.train_step(Bl, LR, flags)


# ------------------------------------------------------------------------------------------ (b) block engine
def block_cases(lib):
    """One case per form and per table shape of the block sweep (block_table_sweep.emulator_slice) at W = 2, Bl = 4 with the
    case's own flags, T and grid (global batch 8 >= every case's B: the sweep's MIN_BN_ROWS / MIN_FINAL_FRAMES conditioning
    holds); the default topology at W = 3 (1 / 3 is no power of two) and W = 4; and one with fewer windows per rank than grid_fwd."""
    out = []
    for c in bts.emulator_slice(lib):
        assert c["B"] <= 8, c
        out.append(dict(id=c["id"], flags=bts.case_flags(c), T=c["T"], W=2, Bl=4, grid=c["grid"], forms=bts.case_forms(c),
                        key=(c["mode"], bts.OPTION_DEFAULTS["bwd_wide"] if "bwd_wide" not in c["options"] else c["options"]["bwd_wide"],
                             bts.form_of(bts.instantiation("bwd_first", c["first"], c["mode"], c["options"])))))
    out.append(dict(id="default-W3-Bl3", flags=ec.DEF, T=60, W=3, Bl=3, grid=0, forms=None, key=None))
    out.append(dict(id="default-W4-Bl2", flags=ec.DEF, T=60, W=4, Bl=2, grid=0, forms=None, key=None))
    out.append(dict(id="default-W2-Bl2-below-grid3", flags=ec.DEF, T=100, W=2, Bl=2, grid=3, forms=None, key=None))
    return out


def block_slice(cases):
    """The emulated slice: one case per (mode, bwd_wide, first-block backward form), the W = 3 default and the one below the grid."""
    seen, out = set(), []
    for c in cases:
        if c["key"] is None:
            if c["W"] != 4:
                out.append(c)
        elif c["key"] not in seen:
            seen.add(c["key"])
            out.append(c)
    return out


def check_sync_bn_block(lib, case, seed=5):
    flags, T, W, Bl, grid = case["flags"], case["T"], case["W"], case["Bl"], case["grid"]
    t0 = time.time()
    B = W * Bl
    om = ec.perturbed_oracle(T, flags=flags)
    lay = MixedNetLayout(flags, T)
    p0, s0 = lay.pack(om.get_weights())
    x, y, w = batch(np.random.default_rng(seed), B, T)
    taps = {}
    om.logits(x, True, taps=taps)
    a0_shape = (Bl,) + tuple(taps["conv1.pre"].shape[1:])

    def make_rank(r):
        _, eng = ec.make_engine(lib, T, Bl, None, flags=flags)
        eng.set_params(p0)
        eng.set_bn_state(s0)
        if grid:
            for k in ("grid_fwd", "grid_bwd", "grid_head"):
                eng.set_option(k, grid)
        return eng

    def script(eng, r, final):
        _step(eng, Bl, r, x, y, w)
        return ec.mixednet_step_reads(eng, lay, Bl, flags, a0_shape) if final else None

    reads, ex = replay(W, make_rank, script, sync_bn=True)
    # the statistics of every block forward and backward (sums and sums of squares / the two gradient sums: 2 * C floats),
    # then the whole flat gradient in one bucket
    widths = [b.cout for b in lay.blocks]
    assert ex.calls == [(2 * c, IN_ORDER) for c in widths + widths[::-1]] + [(lay.n_params, IN_ORDER)], ex.calls
    got = ec.merge_rank_reads(reads)
    worst = {}
    ec.compare_mixednet_step(got, B, lay, om, taps, x, y, w, LR, flags, 0, worst)
    assert np.median(worst["l2s"]) <= ec._mixednet_tols(flags)[3], np.median(worst["l2s"])
    return _record(t0, ex, worst["ratio"])


# ------------------------------------------------------------------------------------------ (b) graph engine
def graph_cases():
    """INC with the fused heads planar, row-stored (the only route to gconv_bwd_kernel<10, 10, GSh3> / <16, 16, GSh7>: a slice
    of the row-stored heads, run singly because sync-BN takes the twins apart) and unfused; INC_VARIANT (sub-spectral groups,
    dilation, two stem layers); three MixedNets on the graph kernels (plain, residual, attention + pooled head)."""
    att_pool = [f for f in ec.GRAPH_MIXEDNET_HEADS if f["spatial_attention"] and f["pooled"] and not f["max_pool"]][0]
    return [gts._case("inc-fused-planar", "inception", ec.INC, 100, 3, 0, fuse_heads=True),
            gts._case("inc-fused-rows", "inception", ec.INC, 100, 2, 0, options={"graph_planar": 0}, fuse_heads=True),
            gts._case("inc-unfused", "inception", ec.INC, 100, 2, 0, fuse_heads=False),
            gts._case("inc-variant", "inception", ec.INC_VARIANT, 100, 3, 0),
            gts._case("graph-mixednet", "mixednet", ec.GRAPH_MIXEDNET, 100, 3, 0),
            gts._case("graph-mixednet-residual", "mixednet", ec.GRAPH_MIXEDNET_RESIDUAL, 100, 2, 0),
            gts._case("graph-mixednet-att-pool", "mixednet", att_pool, 100, 3, 0)]


GRAPH_SLICE = ("inc-fused-rows", "graph-mixednet")   # the emulated slice
GRAPH_W = 2


def declared_graph_kernels():
    """What the cases launch, as graph_table_sweep restates a sync-BN rank's route ("pairing off", finalize launches everywhere)."""
    out = set()
    for c in graph_cases():
        out |= set(gts.case_kernels(c, sync_bn=True))
    return out


def _graph_route(lib, case, lay, new_engine):
    """The launch names of one rank's step under option "profile", with a hook that reduces nothing (the route does not depend on
    the data)."""
    eng = new_engine()
    try:
        eng.set_option("profile", 1)
        eng.set_allreduce_hook(lambda ptr, n, flags: None, GRAPH_W, sync_bn=True, reduce_grads=True)
        B = case["B"]
        rng = np.random.default_rng(5)
        eng.set_batch(ec.synth_x(rng, B, case["T"]))
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), np.ones(B, np.float32))
        if case["kind"] == "inception":
            eng.set_dropout_mask(np.ones((B, lay.t_last * lay.c_last), np.float32))
        eng.train_step(B, LR)
        eng.synchronize()
        return gts.route_of_profile([n for n, _ in eng.profile_read()])
    finally:
        eng.close()


def check_sync_bn_graph(lib, case, seed=7):
    """`case`: of graph_cases(); its B is the windows per rank."""
    t0 = time.time()
    W, Bl, T, flags = GRAPH_W, case["B"], case["T"], case["flags"]
    B = W * Bl
    inception = case["kind"] == "inception"
    rng = np.random.default_rng(seed)
    if inception:
        om = ec.perturbed_inception_oracle(T, flags)
        lay = InceptionLayout(flags, T, fuse_heads=case["fuse_heads"])
    else:
        om = ec.perturbed_oracle(T, flags=flags)
        lay = GraphMixedNetLayout(flags, T)
    p0, s0 = lay.pack(om.get_weights())
    near_zero = 1
    while near_zero:
        x, y, w = batch(rng, B, T)
        # the near-zero-unit condition of check_graph_mixednet(strict), on the oracle: redraw the batch until no unit sits
        # within float32 rounding of a ReLU zero or an attention tie (Inception imposes the engine's decisions instead)
        near_zero, zabs = (0, None) if inception else ec.graph_mixednet_near_zero(om, flags, x)
    keep = (rng.random((B, lay.t_last * lay.c_last)) >= flags["dropout"]).astype(np.float32) if inception else None

    def new_engine():
        eng = native.Engine(lib=lib, **lay.engine_args(Bl))
        if not inception:
            eng.set_grad_mask(lay.grad_mask())
        eng.set_params(p0)
        eng.set_bn_state(s0)
        for k, v in case["options"].items():
            eng.set_option(k, v)
        return eng

    def script(eng, r, final):
        _step(eng, Bl, r, x, y, w, keep)
        if not final:
            return None
        return ec.inception_step_reads(eng, lay, Bl) if inception else ec.graph_mixednet_step_reads(eng, Bl)

    reads, ex = replay(W, lambda r: new_engine(), script, sync_bn=True)
    assert all(f == IN_ORDER for _, f in ex.calls) and ex.calls[-1] == (lay.n_params, IN_ORDER), ex.calls
    n_bn = sum(1 for o in gts.case_ctx(case, sync_bn=True)["G"] if o["norm"] == "bn")
    assert len(ex) == 2 * n_bn + 1, (len(ex), n_bn)
    got = ec.merge_rank_reads(reads)
    l2s = []
    if inception:
        ec.compare_inception_step(got, B, lay, om, x, y, w, keep, LR, 0, l2s)
        ratio = float(np.median(l2s)) / 2e-5
    else:
        loss_slack = float(np.sum(w * 1.2e-7 * np.exp(np.minimum(zabs, 16.0))) / B)
        ec.compare_graph_mixednet_step(got, B, lay, om, x, y, w, LR, 0, l2s, 0, loss_slack)
        ratio = float(np.median(l2s)) / 2e-5
    assert np.median(l2s) <= 2e-5, np.median(l2s)
    # what ran is what graph_table_sweep declares for a sync-BN rank
    want = gts.case_route(case, sync_bn=True)
    route = _graph_route(lib, case, lay, new_engine)
    assert route == want, "%s\nprofiled route %s\ndeclared route %s" % (case["id"], " ".join(route), " ".join(want))
    return _record(t0, ex, ratio)


# ------------------------------------------------------------------------------------------ (c) throughput mode
def check_throughput_composition(lib, kind, W=2, Bl=3, T=60, seed=3):
    """Rank-local BatchNorm.  kind "mixednet": the default MixedNet on the block engine; "inception": INC on the graph engine."""
    t0 = time.time()
    B = W * Bl
    rng = np.random.default_rng(seed)
    x, y, w = batch(rng, B, T)
    if kind == "mixednet":
        om = ec.perturbed_oracle(T)
        lay = MixedNetLayout(ec.DEF, T)
        keep = None
    else:
        om = ec.perturbed_inception_oracle(T, ec.INC)
        lay = InceptionLayout(ec.INC, T)
        keep = (rng.random((B, lay.t_last * lay.c_last)) >= ec.INC["dropout"]).astype(np.float32)
    p0, s0 = lay.pack(om.get_weights())

    def new_engine():
        eng = native.Engine(lib=lib, **lay.engine_args(Bl))
        if kind == "mixednet":
            eng.set_grad_mask(lay.grad_mask())
        eng.set_params(p0)
        eng.set_bn_state(s0)
        return eng

    def reads(eng):
        return dict(grads=eng.get_grads(), params=eng.get_params(), state=eng.get_bn_state())

    def script(eng, r):
        _step(eng, Bl, r, x, y, w, keep)
        return reads(eng)

    def with_buckets(n):
        def make_rank(r):
            eng = new_engine()
            eng.set_option("grad_buckets", n)
            return eng
        return replay(W, make_rank, script, sync_bn=False)

    one, ex1 = with_buckets(1)
    two, ex2 = with_buckets(2)
    assert ex1.calls == [(lay.n_params, IN_ORDER)], ex1.calls
    if kind == "mixednet":   # the deferred bucket: [blocks 3, 4 + dense], as test_local_bn_two_ranks_with_product_kernels derives it
        assert [f for _, f in ex2.calls] == [DEFERRED, IN_ORDER, FLUSH], ex2.calls
        assert ex2.calls[0][0] + ex2.calls[1][0] == lay.n_params and ex2.calls[2][0] == 0 and min(ex2.calls[0][0], ex2.calls[1][0]) > 0, ex2.calls
        segs = lay.segments()
        n_tail = sum(n for _, n in segs[[name for name, _ in segs].index("b2.dw.kernel"):])
        assert ex2.calls[0][0] == n_tail, (ex2.calls, n_tail)
    else:   # the graph engine assembles its gradient in one range: "grad_buckets" 2 is accepted and changes nothing
        assert ex2.calls == ex1.calls, ex2.calls
    # the pieces, on plain engines (no hook): every rank's NO_APPLY gradient and its own single-device step
    total, states = None, []
    for r in range(W):
        eng = new_engine()
        _step(eng, Bl, r, x, y, w, keep, flags=native.STEP_NO_APPLY)
        g = eng.get_grads().copy()
        total = g if total is None else total + g   # float32, rank order
        eng.close()
        eng = new_engine()
        _step(eng, Bl, r, x, y, w, keep)
        states.append(eng.get_bn_state().copy())
        eng.close()
    eng = new_engine()
    _step(eng, Bl, 0, x, y, w, keep, flags=native.STEP_NO_APPLY)   # (Adam's first step from zero moments; the gradient is replaced)
    eng.synchronize()
    _write_grads(eng, total)
    eng.apply_gradients(LR, 1.0 / W)
    params = eng.get_params().copy()
    eng.close()
    for r in range(W):
        for k in ("grads", "params", "state"):
            assert two[r][k].tobytes() == one[r][k].tobytes(), "rank %d %s: 2 buckets differ from 1 bucket" % (r, k)
        assert one[r]["grads"].tobytes() == total.tobytes(), "rank %d: reduced gradient differs from the sum of the ranks' NO_APPLY gradients by %.3g" % (
            r, np.abs(one[r]["grads"] - total).max())
        assert one[r]["params"].tobytes() == params.tobytes(), "rank %d: parameters differ from apply_gradients(lr, 1 / W) on the sum by %.3g lr" % (
            r, np.abs(one[r]["params"] - params).max() / LR)
        assert one[r]["state"].tobytes() == states[r].tobytes(), "rank %d: BN state differs from its single-device step" % r
    assert one[0]["state"].tobytes() != one[1]["state"].tobytes()
    return _record(t0, ex2, 0.0, runs_total=ex1.runs + ex2.runs)


def _write_grads(eng, values):
    """`values` into the engine's flat gradient (host memory of an emulated library, HBM otherwise)."""
    import torch
    mem = Memory(eng)
    v = mem.view(eng.device_ptr(native.BUF_GRADS), eng.n_params)
    src = torch.from_numpy(np.ascontiguousarray(values, np.float32))
    mem.overwrite(v, src if mem.host else src.to(mem.device))
    if not mem.host:
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ (d) step features
def _feature_inputs(steps, W, Bl, T, extra=0, seed=3):
    rng = np.random.default_rng(seed)
    x = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(steps)])
    px = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(extra)]) if extra else None
    y = (rng.random((steps, W * Bl)) < 0.5).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=(steps, W * Bl)).astype(np.float32)
    return x, y, w, px


def check_weight_qat(lib, W=2, Bl=3, T=60, steps=3):
    """Weight QAT with sync-BN and 2 buckets over 3 steps: the assertions of tests/test_weight_qat_parallel_gloo.py."""
    import weight_qat_checks as wq
    from microwakeword_amd import qat
    t0 = time.time()
    x, y, w, _ = _feature_inputs(steps, W, Bl, T)
    om = ec.perturbed_oracle(T)
    lay = MixedNetLayout(ec.DEF, T)
    p0, s0 = lay.pack(om.get_weights())

    def make(bl):
        _, eng = ec.make_engine(lib, T, bl, None)
        eng.set_params(p0)
        eng.set_bn_state(s0)
        eng.set_option("grad_buckets", 2)
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)
        return eng

    def run(eng, r, bl, final=True):
        for s in range(steps):
            _step(eng, bl, r, x[s], y[s], w[s])
            if final:
                wq.assert_shadow(eng, lay, "rank %d after step %d" % (r, s + 1))
        m, v, step = eng.get_opt_state()
        return dict(params=eng.get_params(), state=eng.get_bn_state(), grads=eng.get_grads(), shadow=eng.get_forward_params(), m=m, v=v, step=step)

    (a, b), ex = replay(W, lambda r: make(Bl), lambda eng, r, final: run(eng, r, Bl, final), sync_bn=True)
    eng = make(W * Bl)
    one = run(eng, 0, W * Bl)
    eng.close()
    assert int(a["step"]) == int(b["step"]) == int(one["step"]) == steps
    for k in ("params", "state", "grads", "shadow", "m", "v"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not np.array_equal(a["shadow"], a["params"])
    # the single rank's on the whole batch: two engine runs are within twice engine_checks' per-step bounds, over `steps` steps
    well = np.abs(one["grads"]) > 1e-4 * np.abs(one["grads"]).max()
    diff = np.abs(a["params"] - one["params"])
    state_err = np.abs(a["state"] - one["state"]).max()
    state_bound = steps * 2 * 1e-5 * max(1.0, np.abs(one["state"]).max())
    assert diff[well].max() <= steps * 2 * 0.05 * LR and diff.max() <= steps * 2 * 2.0 * LR, (diff[well].max() / LR, diff.max() / LR)
    assert state_err <= state_bound
    return _record(t0, ex, max(diff[well].max() / (steps * 2 * 0.05 * LR), state_err / state_bound))


def check_weight_ema(lib, W=2, Bl=3, T=60, steps=4, decay=0.9, every_steps=(1, 2)):
    """The weight average behind sync-BN and the two-bucket exchange: the assertions of tests/test_weight_ema_parallel_gloo.py."""
    from microwakeword_amd import averaging
    t0 = time.time()
    x, y, w, _ = _feature_inputs(steps, W, Bl, T)
    om = ec.perturbed_oracle(T)
    lay = MixedNetLayout(ec.DEF, T)
    p0, s0 = lay.pack(om.get_weights())
    n_ex = runs = 0
    for every in every_steps:
        def make_rank(r):
            _, eng = ec.make_engine(lib, T, Bl, None)
            eng.set_params(p0)
            eng.set_bn_state(s0)
            eng.set_option("grad_buckets", 2)
            eng.set_weight_ema(decay, every)
            return eng

        def script(eng, r):
            masters = []
            for s in range(steps):
                _step(eng, Bl, r, x[s], y[s], w[s])
                masters.append(eng.get_params())
            ema, updates = eng.get_ema_state()
            return dict(masters=np.stack(masters), ema=ema, updates=updates, step=eng.get_opt_state()[2])

        (a, b), ex = replay(W, make_rank, script, sync_bn=True)
        n_ex, runs = n_ex + len(ex), runs + ex.runs
        assert int(a["step"]) == int(b["step"]) == steps and int(a["updates"]) == int(b["updates"]) == steps // every
        assert a["masters"].tobytes() == b["masters"].tobytes()
        assert a["ema"].tobytes() == b["ema"].tobytes()
        want, n = averaging.ema_fold(list(a["masters"]), decay, every)
        assert n == steps // every and a["ema"].tobytes() == want.tobytes()
        assert a["ema"].tobytes() != a["masters"][-1].tobytes()
    return dict(exchanges=n_ex, runs=runs, seconds=time.time() - t0, ratio=0.0)


def check_bn_reestimate_sync(lib, W=2, Bl=3, T=60, K=2, decay=0.9):
    """BN re-estimation with sync-BN ON (forward_stat_source reads the row of global sums): one step, then begin / K x batch /
    commit.  The ranks end byte-equal, and the statistics are those of the WHOLE batches: bn_reestimate_checks' float64
    restatement on the global batches, at that file's bound."""
    import bn_reestimate_checks as bn
    from microwakeword_amd import averaging
    assert T == bn.T
    t0 = time.time()
    x, y, w, px = _feature_inputs(1, W, Bl, T, extra=K)
    om = ec.perturbed_oracle(T)
    lay = MixedNetLayout(ec.DEF, T)
    p0, s0 = lay.pack(om.get_weights())

    def make_rank(r):
        _, eng = ec.make_engine(lib, T, Bl, None)
        eng.set_params(p0)
        eng.set_bn_state(s0)
        eng.set_weight_ema(decay, 1)
        return eng

    def script(eng, r):
        _step(eng, Bl, r, x[0], y[0], w[0])
        eng.bn_reestimate_begin()
        for k in range(K):
            eng.set_batch(px[k, r * Bl:(r + 1) * Bl])
            eng.bn_reestimate_batch(Bl)
        eng.bn_reestimate_commit()
        got, valid = eng.get_ema_bn_state()
        assert valid
        return dict(ema_bn=got, vec=bn.averaged_vector(lay, "block", eng), state=eng.get_bn_state())

    reads, ex = replay(W, make_rank, script, sync_bn=True)
    for r in range(1, W):
        for k in ("ema_bn", "vec", "state"):
            assert reads[r][k].tobytes() == reads[0][k].tobytes(), (r, k)
    # the host-side rank mean (DataParallel.average_ema_bn_state is a no-op under sync-BN): of identical vectors, themselves
    mean = averaging.bn_rank_mean([g["ema_bn"] for g in reads])
    assert mean.tobytes() == reads[0]["ema_bn"].tobytes()
    assert reads[0]["ema_bn"].tobytes() != reads[0]["state"].tobytes()
    ref = np.asarray(bn.oracle_statistics(lay, "block", reads[0]["vec"], list(px), W * Bl, flags=ec.DEF), np.float64)
    err, bound = np.abs(reads[0]["ema_bn"].astype(np.float64) - ref).max(), 1e-5 * max(1.0, np.abs(ref).max())
    print("sync-BN re-estimation, W %d: max |ema_bn - oracle on the global batches| = %.3g (bound %.3g)" % (W, err, bound))
    assert err <= bound, (err, bound)
    return _record(t0, ex, err / bound)


def report(case_id, rec):
    """One line per case, as profiles/exchange_replay_results.txt holds them."""
    print("exchange-replay %-40s exchanges %3d runs %4d seconds %6.2f worst error / bound %.3f" % (
        case_id, rec["exchanges"], rec.get("runs_total", rec["runs"]), rec["seconds"], rec["ratio"]), flush=True)
