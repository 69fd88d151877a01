"""Checks of BatchNorm re-estimation for the weight average (``mww_bn_reestimate_*``, csrc/kernels_bnre.hip.h,
``microwakeword_amd/averaging.py``), shared by tests/test_bn_reestimate_emulated.py (tests/hipemu) and
tests/test_bn_reestimate_gpu.py, the same shapes on both: the three small models of tests/weight_qat_checks.py (block kernels,
graph kernels, Inception with SubSpectralNormalization slots), B = 8, T = 60, pass batches of 8 and of 5 (below ``max_batch``:
an ``inv_n`` taken from the wrong batch size shows), K in {1, 2, 3}, under both settings of the ``bn_inline`` option.

Every comparison but the oracle's is byte for byte: the statistics are specified as the forward's own floats, the accumulation
and the commit operation for operation (``averaging.bn_reestimate``).
"""
import os
import random

import numpy as np
import pytest
import torch

import engine_checks as ec
import weight_ema_checks as we
import weight_qat_checks as wq
from microwakeword_amd import averaging, native, qat
from oracle import model_oracle as mo

B, T, KINDS = wq.B, wq.T, wq.KINDS
LR = we.LR
same_bits, all_same = wq.same_bits, wq.all_same
PASS_BATCHES = (8, 5)
INLINE = (1, 0)
# kBnMomentum = 0.99f: the factor a train step blends the batch statistic in with, formed in float32 like the kernels form it
BLEND = np.float32(1.0) - np.float32(0.99)


def xs_of(n, seed=31):
    rng = np.random.default_rng(seed)
    return [ec.synth_x(rng, B, T) for _ in range(n)]


def prepared(lib, kind, inline, steps=3, extra=None, weights=None):
    """an engine of the kind with an installed average that has taken ``steps`` updates"""
    def prepare(eng, lay):
        if weights is not None:
            p, s = lay.pack(weights)
            eng.set_params(p)
            eng.set_bn_state(s)
        eng.set_option("bn_inline", inline)
        if extra is not None:
            extra(eng, lay)
        eng.set_weight_ema(we.DECAY, 1)
    lay, eng = we.start(lib, kind, prepare)
    for b in we.batches(steps):
        we.step(eng, b)
    return lay, eng


def averaged_vector(lay, kind, eng):
    """the averaged model as a master: trainable elements from the average, the rest (masked MixConv taps) from the master"""
    vec = eng.get_params()
    ema, n = eng.get_ema_state()
    assert n > 0
    trainable = lay.grad_mask() != 0 if kind != "inception" else np.ones(vec.size, bool)
    vec[trainable] = ema[trainable]
    return vec


def one_pass(eng, xs, b):
    eng.bn_reestimate_begin()
    for x in xs:
        eng.set_batch(x[:b])
        eng.bn_reestimate_batch(b)
    eng.bn_reestimate_commit()
    got, valid = eng.get_ema_bn_state()
    assert valid and eng.ema_bn_valid()
    return got


def compose(states):
    rows = np.stack(states)
    return averaging.bn_reestimate(rows, rows)[0]   # (the state vector holds means and variances; both commit alike)


def twin_of(lib, kind, inline, master, state, extra=None):
    def prepare(eng, lay):
        eng.set_option("bn_inline", inline)
        if extra is not None:
            extra(eng, lay)
    lay, twin = we.start(lib, kind, prepare)
    twin.set_params(master)
    twin.set_bn_state(state)
    return twin


def diff_report(got, want, what):
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    return "%s: %d of %d statistics differ, first %d: %r vs %r" % (what, bad.size, got.size, bad[0] if bad.size else -1,
                                                                  got[bad[0]] if bad.size else None, want[bad[0]] if bad.size else None)


# ---------------------------------------------------------------------------------------------- (a) composition
def check_composition(lib, kind, inline):
    lay, eng = prepared(lib, kind, inline)
    master_state = eng.get_bn_state()
    xs = xs_of(3)
    for b in PASS_BATCHES:
        singles = [one_pass(eng, [x], b) for x in xs]
        assert not same_bits(singles[0], singles[1])
        for K in (2, 3):
            got = one_pass(eng, xs[:K], b)
            want = compose(singles[:K])
            assert same_bits(got, want), diff_report(got, want, "%s b %d K %d" % (kind, b, K))
            assert same_bits(one_pass(eng, xs[:K], b), got)   # two passes over the same batches: the same bytes
        assert not same_bits(singles[0], one_pass(eng, xs[:1], 13 - b))   # (the other batch size: other statistics)
    assert same_bits(eng.get_bn_state(), master_state)   # the master's moving statistics are never written
    eng.close()
    return eng.n_state


# ---------------------------------------------------------------------------------------------- (b) the forward's own statistics
def check_forwards_own_statistics(lib, kind, inline, extra=None):
    lay, eng = prepared(lib, kind, inline, extra=extra)
    xa = xs_of(1, seed=32)[0]
    rng = np.random.default_rng(6)
    y, w = (rng.random(B) < 0.5).astype(np.float32), np.ones(B, np.float32)
    if extra is not None:
        eng.set_option("ema_forward", 1)
        master = eng.get_forward_params()   # fake_quant(average): the twin's master is that shadow, its own option off
        eng.set_option("ema_forward", 0)
    else:
        master = averaged_vector(lay, kind, eng)
    for b in PASS_BATCHES:
        r = one_pass(eng, [xa], b)
        twin = twin_of(lib, kind, inline, master, np.zeros(eng.n_state, np.float32))
        twin.set_batch(xa[:b])
        twin.set_targets(y[:b], w[:b])
        twin.train_step(b, LR, native.STEP_NO_APPLY)
        got = twin.get_bn_state()
        want = (r * BLEND).astype(np.float32)
        assert same_bits(got, want), diff_report(got, want, "%s inline %d b %d" % (kind, inline, b))
        twin.close()
    eng.close()


# ---------------------------------------------------------------------------------------------- (c) the float64 oracle
def oracle_statistics(lay, kind, vec, xs, b, flags=None):
    """batch mean / biased variance of every BN input at the weights ``vec``, averaged over the batches, in bn_state layout
    (``flags``: of a model other than the kind's own, at the same T)"""
    om = mo.OracleModel("inception" if kind == "inception" else "mixednet", wq.flags_of(kind) if flags is None else flags, T)
    weights = lay.unpack(vec, np.zeros(lay.n_state, np.float32))   # moving statistics zero: new = 0 * 0.99 + stat * (1 - 0.99)
    om.set_weights(weights)
    names = [v.name for v in om.vars]
    assert [tuple(v.value.shape) for v in om.vars] == [s for _, s, _ in lay.keras_vars]
    acc = [np.zeros(s, np.float64) for _, s, _ in lay.keras_vars]
    for x in xs:
        taps = {}
        xt = torch.tensor(x[:b], dtype=torch.float64)
        keep = torch.ones((b, 1), dtype=torch.float64) if kind == "inception" else None
        _, new = om.logits(xt, True, dropout_mask=keep, taps=taps)
        for i, name in enumerate(names):
            if name in new:
                stat = new[name].detach().numpy().astype(np.float64) / (1.0 - mo.BN_MOMENTUM)
                acc[i] += stat
                tap = name.rsplit(".bn.", 1)[0] + ".pre_bn"
                if tap in taps and stat.size == taps[tap].shape[2]:   # a plain BN with a tap of its input: the tap says the same
                    t = taps[tap].detach().numpy().reshape(-1, stat.size)
                    direct = t.mean(0) if name.endswith("moving_mean") else t.var(0)
                    assert np.abs(direct - stat).max() <= 1e-9 * max(1.0, np.abs(direct).max())
    # (the layout packs float32: the reference is rounded once, 6e-8 relative, far inside the bound)
    return lay.pack([a / len(xs) for a in acc])[1]


def check_against_oracle(lib, kind, inline):
    # the bound is the one engine_checks.check_train_steps holds the moving statistics to, so the weights are the ones it
    # starts from: an oracle's initial weights, perturbed (we.start's span five decades: a variance of 385 next to one of
    # 0.006 leaves float32 activations no 1e-5 of the largest statistic)
    om = ec.perturbed_inception_oracle(T, wq.flags_of(kind)) if kind == "inception" else ec.perturbed_oracle(T, flags=wq.flags_of(kind))
    lay, eng = prepared(lib, kind, inline, weights=om.get_weights())
    vec = averaged_vector(lay, kind, eng)
    xs = xs_of(2, seed=33)
    for b in PASS_BATCHES:
        got = one_pass(eng, xs, b)
        ref = np.asarray(oracle_statistics(lay, kind, vec, xs, b), np.float64)
        err, bound = np.abs(got.astype(np.float64) - ref).max(), 1e-5 * max(1.0, np.abs(ref).max())
        print("%s inline %d b %d: max |ema_bn - oracle| = %.3g (bound %.3g)" % (kind, inline, b, err, bound))
        assert err <= bound, (kind, inline, b, err, bound)
    eng.close()


# ---------------------------------------------------------------------------------------------- (d) evaluation is a twin
def check_evaluation_is_a_twin(lib, kind, inline):
    lay, eng = prepared(lib, kind, inline)
    x, y, _ = we.batches(1, seed=8)[0]
    ema_bn = one_pass(eng, xs_of(2, seed=34), 8)
    master_state = eng.get_bn_state()
    assert not same_bits(ema_bn, master_state)
    eng.set_option("ema_forward", 1)
    assert eng.ema_bn_valid()   # (the option does not change what the pass described)
    vec = averaged_vector(lay, kind, eng)
    twin = twin_of(lib, kind, inline, vec, ema_bn)
    stale = twin_of(lib, kind, inline, vec, master_state)
    got, want, old = we.eval_outputs(eng, x, y), we.eval_outputs(twin, x, y), we.eval_outputs(stale, x, y)
    assert all_same(got, want)
    assert not same_bits(old[1], want[1])   # ... which is not what the master's statistics give
    # with the option off the master is read, with its own statistics
    eng.set_option("ema_forward", 0)
    plain = twin_of(lib, kind, inline, eng.get_params(), master_state)
    assert all_same(we.eval_outputs(eng, x, y), we.eval_outputs(plain, x, y))
    for e in (eng, twin, stale, plain):
        e.close()


# ---------------------------------------------------------------------------------------------- (e) observing only
def check_observing_only(lib, kind, inline, graphs=0):
    xs = xs_of(2, seed=35)
    runs = []
    for passes in (False, True):
        def prepare(eng, lay):
            eng.set_option("bn_inline", inline)
            eng.set_weight_ema(we.DECAY, 1)
            if graphs:
                eng.set_option("graphs", 1)
        lay, eng = we.start(lib, kind, prepare)
        outs = []
        for k, b in enumerate(we.batches(5)):
            we.step(eng, b)
            outs.append(eng.read_outputs(B)[0])
            if passes and k in (0, 2, 3):
                one_pass(eng, xs, 8 if k != 2 else 5)
        runs.append((we.snapshot(eng) + eng.get_ema_state(), outs, eng))
    (plain, outs_p, e0), (passed, outs_q, e1) = runs
    assert all(np.all(np.isfinite(a)) for a in plain[:4])
    assert all_same(plain, passed)   # parameters, master bn_state, Adam m / v / step, gradients, the average and its count
    assert all_same(outs_p, outs_q)   # (Inception: the dropout draws of every step)
    e0.close()
    e1.close()


# ---------------------------------------------------------------------------------------------- (f) invalidation
def check_invalidation(lib, kind, inline):
    lay, eng = prepared(lib, kind, inline)
    x, y, _ = we.batches(1, seed=8)[0]
    xs = xs_of(1, seed=36)
    eng.set_option("ema_forward", 1)

    def reads_the_masters():
        assert not eng.ema_bn_valid()
        state, valid = eng.get_ema_bn_state()
        assert not valid and same_bits(state, eng.get_bn_state())
        twin = twin_of(lib, kind, inline, averaged_vector(lay, kind, eng), eng.get_bn_state())
        assert all_same(we.eval_outputs(eng, x, y), we.eval_outputs(twin, x, y))
        twin.close()
    reads_the_masters()   # before any pass
    one_pass(eng, xs, 8)
    we.step(eng, we.batches(4)[3])   # the next update of the average
    reads_the_masters()
    one_pass(eng, xs, 8)
    ema, n = eng.get_ema_state()
    eng.set_ema_state(ema, n)
    reads_the_masters()
    one_pass(eng, xs, 8)
    eng.set_weight_qat_map(*qat.channel_map(lay))   # the map
    assert not eng.ema_bn_valid()
    one_pass(eng, xs, 8)
    eng.set_option("weight_qat", 1)   # the option
    assert not eng.ema_bn_valid()
    one_pass(eng, xs, 8)
    eng.set_option("weight_qat", 1)   # (unchanged: nothing an evaluation reads moved)
    assert eng.ema_bn_valid()
    eng.set_option("weight_qat", 0)
    reads_the_masters()
    # an update closes a pass in progress
    eng.bn_reestimate_begin()
    eng.set_batch(xs[0])
    eng.bn_reestimate_batch(B)
    we.step(eng, we.batches(5)[4])
    with pytest.raises(native.NativeError, match="error -4: .*commit without"):
        eng.bn_reestimate_commit()
    one_pass(eng, xs, 8)
    eng.set_weight_ema(we.DECAY, 2)   # installing anew
    assert not eng.ema_bn_valid()
    eng.close()


# ---------------------------------------------------------------------------------------------- (g) with weight_qat
def qat_on(eng, lay):
    eng.set_weight_qat_map(*qat.channel_map(lay))
    eng.set_option("weight_qat", 1)


def check_with_weight_qat(lib, kind, inline):
    lay, eng = prepared(lib, kind, inline, extra=qat_on)
    xs = xs_of(2, seed=37)
    eng.set_option("ema_forward", 1)
    shadow = eng.get_forward_params()
    ema, n = eng.get_ema_state()
    assert same_bits(shadow, qat.forward_params_reference(lay, ema)) and not same_bits(shadow, ema)
    got = one_pass(eng, xs, 8)
    # a twin whose master - and whose average - is that shadow, its own option off
    twin = twin_of(lib, kind, inline, shadow, eng.get_bn_state())
    twin.set_weight_ema(we.DECAY, 1)
    twin.set_ema_state(shadow, 1)
    want = one_pass(twin, xs, 8)
    assert same_bits(got, want), diff_report(got, want, kind)
    plain = twin_of(lib, kind, inline, ema, eng.get_bn_state())
    plain.set_weight_ema(we.DECAY, 1)
    plain.set_ema_state(ema, 1)
    assert not same_bits(one_pass(plain, xs, 8), got)   # ... not the statistics of the unquantized average
    for e in (eng, twin, plain):
        e.close()
    check_forwards_own_statistics(lib, kind, inline, extra=qat_on)


# ---------------------------------------------------------------------------------------------- (h) the windows form
def check_windows_form(lib, kind, inline):
    lay, eng = prepared(lib, kind, inline)
    rng = np.random.default_rng(9)
    n = 2 * B
    u16 = rng.integers(0, 26 * 25, size=(n // 2 + 1) * T * 40).astype(np.uint16)
    f32 = (rng.random(((n // 2 + 1) * T, 40)) * 26.0).astype(np.float32).reshape(-1)
    eng.upload_store(0, u16)
    eng.upload_store(1, f32)
    pads = rng.integers(0, 7, size=n)
    pads[0], pads[n - 1] = 0, T // 2
    win = np.zeros(n, native.WINDOW_DTYPE)
    rows = np.zeros((n, T, 40), np.float32)
    for i in range(n):
        store, pad = i % 2, int(pads[i])
        src = int(rng.integers(0, (n // 2 + 1) * T - (T - pad) + 1)) * 40
        win[i] = (store, pad, T - pad, 0, src)
        flat = u16.astype(np.float32) * np.float32(0.0390625) if store == 0 else f32
        rows[i, pad:] = flat[src:src + (T - pad) * 40].reshape(T - pad, 40)
    master_state = eng.get_bn_state()
    eng.bn_reestimate_windows(win, B)
    got, valid = eng.get_ema_bn_state()
    assert valid
    want = one_pass(eng, [rows[:B], rows[B:]], B)
    assert same_bits(got, want), diff_report(got, want, kind)
    # refused lists leave the statistics of the last pass in place
    for bad, batch in ((win[:B + 3], B), (win[:0], B), (win[:5], B), (win, B + 1)):
        with pytest.raises(native.NativeError, match="error -1: .*(multiple|batch|arguments)"):
            eng.bn_reestimate_windows(bad, batch)
    outside = win.copy()
    outside[3]["src_elem"] = u16.size
    with pytest.raises(native.NativeError, match="error -1: .*past the end"):
        eng.bn_reestimate_windows(outside, B)
    state, valid = eng.get_ema_bn_state()
    assert valid and same_bits(state, want) and same_bits(eng.get_bn_state(), master_state)
    # five windows per batch, fifteen windows
    eng.bn_reestimate_windows(win[:15], 5)
    got5 = eng.get_ema_bn_state()[0]
    assert same_bits(got5, one_pass(eng, [rows[0:5], rows[5:10], rows[10:15]], 5))
    eng.close()


# ---------------------------------------------------------------------------------------------- (i) refusals
def check_refusals(lib, kind):
    bs = we.batches(3)
    lay, fresh = we.start(lib, kind)
    we.step(fresh, bs[0])
    want = we.snapshot(fresh)
    fresh.close()

    def no(call, word, code=-1):
        with pytest.raises(native.NativeError, match="error %d: .*%s" % (code, word)):
            call()
    lay, eng = we.start(lib, kind)
    S = eng.n_state
    x = xs_of(1)[0]
    eng.set_batch(x)
    win = np.array([(0, 0, T, 0, i * T * 40) for i in range(B)], native.WINDOW_DTYPE)
    eng.upload_store(0, x.reshape(-1))
    # no average installed
    no(eng.bn_reestimate_begin, "weight average")
    no(lambda: eng.bn_reestimate_windows(win, B), "weight average")
    no(eng.get_ema_bn_state, "weight average")
    no(lambda: eng.set_ema_bn_state(np.zeros(S, np.float32)), "weight average")
    no(lambda: eng.bn_reestimate_batch(B), "no pass is open", -4)
    no(eng.bn_reestimate_commit, "commit without", -4)
    # installed, no update taken yet
    eng.set_weight_ema(we.DECAY, 1)
    no(eng.bn_reestimate_begin, "taken an update")
    no(lambda: eng.bn_reestimate_windows(win, B), "taken an update")
    assert not eng.ema_bn_valid()
    we.step(eng, bs[0])
    assert all_same(we.snapshot(eng), want)   # the context is usable: the step of a fresh context
    # a commit without a batch; a batch size out of range
    eng.bn_reestimate_begin()
    no(eng.bn_reestimate_commit, "commit without", -4)
    no(lambda: eng.bn_reestimate_batch(0), "batch size")
    no(lambda: eng.bn_reestimate_batch(B + 1), "batch size")
    assert not eng.ema_bn_valid()
    eng.set_batch(x)
    state = one_pass(eng, [x], B)
    # a wrong n in the get / set pair
    for n in (S - 1, S + 1):
        no(lambda: eng.nl.check(eng.nl.lib.mww_get_ema_bn_state(eng.h, None, n, None)), "size")
        no(lambda: eng.set_ema_bn_state(np.zeros(n, np.float32)), "size")
    got, valid = eng.get_ema_bn_state()
    assert valid and same_bits(got, state)
    # validity survives a get / set round trip: into a context whose statistics were invalidated
    we.step(eng, bs[1])
    assert not eng.ema_bn_valid()
    eng.set_ema_bn_state(state)
    got, valid = eng.get_ema_bn_state()
    assert valid and same_bits(got, state)
    we.step(eng, bs[2])   # ... and the context trains on
    assert not eng.ema_bn_valid()
    eng.set_weight_ema(0.0)
    no(eng.get_ema_bn_state, "weight average")
    eng.close()


# ---------------------------------------------------------------------------------------------- (j) the loop
SAMPLES = 40   # cut down to two batches of 16


def loop_config(tmp_path, name, bn="default", **over):
    if bn == "default":
        bn = dict(samples=SAMPLES, seed=0)
    amap = dict(decay=we.DECAY, first_step=we.FIRST_STEP)
    if bn is not None:
        amap["bn_reestimate"] = bn
    return we.loop_config(tmp_path, name, averaging_map=amap, **over)


class PassRecorder:
    """records the result of every re-estimation pass and, at every window evaluation, whether it stood on valid statistics"""

    def __init__(self, monkeypatch):
        self.passes, self.evaluated_valid, self.windows = [], [], []
        rec = self
        plain_pass, plain_eval = native.Engine.bn_reestimate_windows, native.Engine.evaluate_windows

        def bn_reestimate_windows(eng, windows, batch):
            plain_pass(eng, windows, batch)
            rec.passes.append((eng.get_opt_state()[2], eng.get_ema_bn_state()[0]))
            rec.windows.append((np.array(windows), batch))

        def evaluate_windows(eng, *a, **k):
            rec.evaluated_valid.append((eng.get_opt_state()[2], eng.ema_bn_valid()))
            plain_eval(eng, *a, **k)
        monkeypatch.setattr(native.Engine, "bn_reestimate_windows", bn_reestimate_windows)
        monkeypatch.setattr(native.Engine, "evaluate_windows", evaluate_windows)

    def clear(self):
        del self.passes[:], self.evaluated_valid[:], self.windows[:]


def check_loop(lib, tmp_path, caplog, monkeypatch):
    import mining_checks as mc
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    from microwakeword_amd import mixednet
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    rec, pr = we.Recorder(monkeypatch), PassRecorder(monkeypatch)
    cfg = loop_config(tmp_path, "bnre")
    model, fh = smc.run_loop(lib, cfg)
    lay = model.layout
    # one pass per boundary (the average is on from step 3), over the same two whole batches of seeded windows
    assert [s for s, _ in pr.passes] == svc.BOUNDARIES
    assert all(w.shape[0] == 2 * smc.B_LOOP and b == smc.B_LOOP for w, b in pr.windows)
    assert all(w.tobytes() == pr.windows[0][0].tobytes() for w, _ in pr.windows)
    assert pr.windows[0][0].tobytes() == fh.draw_seeded_windows(SAMPLES, smc.T_LOOP, 0)[:2 * smc.B_LOOP].tobytes()
    # validation ran on them
    assert pr.evaluated_valid and all(valid for s, valid in pr.evaluated_valid if s >= we.FIRST_STEP)
    emas, ema, updates = {}, None, 0
    for k in range(we.FIRST_STEP, smc.STEPS + 1):
        ema, updates = averaging.ema_fold([rec.masters[k - 1]], we.DECAY, 1, k, ema, updates)
        emas[k] = ema
    at = {}
    for (k, ema_bn) in pr.passes:
        assert not same_bits(ema_bn, rec.states[k - 1])
        at[k] = [w.tobytes() for w in we.averaged_variables(lay, rec.masters[k - 1], ema_bn, emas[k])]
        assert we.arrays_of(svc.weights_at(cfg, k)) == at[k], k
    assert we.arrays_of(os.path.join(cfg["train_dir"], "last_weights.weights.h5")) == at[smc.STEPS]
    assert we.arrays_of(os.path.join(cfg["train_dir"], "best_weights.weights.h5")) in list(at.values())
    # the pass is the engine's: the recorded result is the three-call form on the host rows of the same windows
    from microwakeword_amd.quantize import window_host_rows
    rows = window_host_rows(fh, pr.windows[0][0]).reshape(2, smc.B_LOOP, smc.T_LOOP, 40)
    assert model.engine.ema_bn_valid()
    assert same_bits(one_pass(model.engine, [rows[0], rows[1]], smc.B_LOOP), pr.passes[-1][1])
    # the restore checkpoint carries the master with the master's statistics; Model.get_weights inside the context the average's
    ckpt = os.path.join(cfg["train_dir"], "restore", "ckpt")
    assert we.arrays_of(ckpt + ".weights") == [w.tobytes() for w in lay.unpack(rec.masters[-1], rec.states[-1])]
    with np.load(ckpt + ".opt.npz") as z:
        assert sorted(z.files) == ["ema", "ema_decay", "ema_every_steps", "ema_updates", "lr", "m", "step", "v"]   # unchanged
    with model.averaged_weights():
        assert [w.tobytes() for w in model.get_weights()] == at[smc.STEPS]
        with model.master_weights():
            assert [w.tobytes() for w in model.get_weights()] == we.arrays_of(ckpt + ".weights")
    assert [w.tobytes() for w in model.get_weights()] == we.arrays_of(ckpt + ".weights")
    # stopped after step 8 and restored: the statistics are re-derived at the next boundary, which the run reproduces
    cut = loop_config(tmp_path, "cut", training_steps=[6, 2])
    full_pass = pr.passes[-1][1]
    rec.clear()
    pr.clear()
    smc.run_loop(lib, cut)
    rest = dict(cut, training_steps=[4], learning_rates=[cfg["learning_rates"][1]])
    state = mc.rng_state()
    random.seed(1)
    np.random.seed(1)
    restored = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=99, max_batch=64)
    fh2 = FeatureHandler(rest, engine=restored.engine)
    random.setstate(state[0])
    np.random.set_state(state[1])
    pr.clear()
    tr.train(restored, rest, fh2, verbose=False)
    assert [s for s, _ in pr.passes] == [smc.STEPS]
    assert same_bits(pr.passes[0][1], full_pass)
    for name in ("last_weights.weights.h5", os.path.join("restore", "ckpt.weights")):
        assert we.arrays_of(os.path.join(cut["train_dir"], name)) == we.arrays_of(os.path.join(cfg["train_dir"], name)), name


def check_loop_without_the_key(lib, tmp_path, monkeypatch):
    """weight_averaging without bn_reestimate: no pass, and the files carry the master's moving statistics, as before"""
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    rec, pr = we.Recorder(monkeypatch), PassRecorder(monkeypatch)
    cfg = loop_config(tmp_path, "nokey", bn=None)
    model, _ = smc.run_loop(lib, cfg)
    lay = model.layout
    assert not pr.passes and not any(valid for _, valid in pr.evaluated_valid) and not model.engine.ema_bn_valid()
    ema, updates = None, 0
    for k in range(we.FIRST_STEP, smc.STEPS + 1):
        ema, updates = averaging.ema_fold([rec.masters[k - 1]], we.DECAY, 1, k, ema, updates)
        if k in svc.BOUNDARIES:
            want = [w.tobytes() for w in we.averaged_variables(lay, rec.masters[k - 1], rec.states[k - 1], ema)]
            assert we.arrays_of(svc.weights_at(cfg, k)) == want, k


BAD_MAPPINGS = ((dict(samples=0), "samples"), (dict(samples=-4), "samples"), (dict(samples=2.5), "samples"), (dict(samples=True), "samples"),
                (dict(samples="64"), "samples"), (dict(seed=0), "samples"), (dict(samples=64, seed=-1), "seed"), (dict(samples=64, seed=1.5), "seed"),
                (dict(samples=64, batches=2), "batches"), (64, "mapping"))


def check_bad_settings(lib, tmp_path):
    import stream_mine_checks as smc
    for bad, word in BAD_MAPPINGS:
        with pytest.raises(ValueError, match="weight_averaging.*" + word):
            averaging.parse_config({"weight_averaging": dict(decay=0.9, first_step=1, bn_reestimate=bad)})
    got = averaging.parse_config({"weight_averaging": dict(decay=0.9, first_step=1, bn_reestimate=dict(samples=np.int64(64)))})
    assert got["bn_reestimate"] == {"samples": 64, "seed": 0}
    assert "bn_reestimate" not in averaging.parse_config({"weight_averaging": dict(decay=0.9, first_step=1)})
    # refused before step 0: a bad value, and fewer samples than one batch
    for bn, word in ((dict(samples=0), "samples"), (dict(samples=smc.B_LOOP - 1), "less than one batch")):
        cfg = loop_config(tmp_path, "bad%d" % bn["samples"], bn=bn)
        with pytest.raises(ValueError, match="weight_averaging.*" + word):
            smc.run_loop(lib, cfg)
        assert not os.path.exists(os.path.join(cfg["train_dir"], "restore")) and not os.path.exists(os.path.join(cfg["train_dir"], "last_weights.weights.h5.npz"))
