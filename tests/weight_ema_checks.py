"""Checks of weight averaging (``mww_set_weight_ema`` / the ``ema_forward`` option of the context core, csrc/kernels_ema.hip.h,
``microwakeword_amd/averaging.py``), shared by tests/test_weight_ema_emulated.py (tests/hipemu) and tests/test_weight_ema_gpu.py,
the same shapes on both: the three small models of tests/weight_qat_checks.py (both engines; parameter counts that are neither
multiples of four nor of a workgroup).

Every comparison is byte for byte: the update is specified operation for operation (``averaging.ema_update``), and everything
else is "the same launches on the same inputs".
"""
import logging
import os
import random

import numpy as np
import pytest

import engine_checks as ec
import weight_qat_checks as wq
from microwakeword_amd import averaging, native, qat

B, T, KINDS = wq.B, wq.T, wq.KINDS
LR, DECAY = 1e-2, 0.9
same_bits, all_same = wq.same_bits, wq.all_same


def start(lib, kind, prepare=None):
    """an engine of the kind on fixed weights (wq.three_steps' start)"""
    lay, eng = wq.new_engine(lib, kind)
    p, s = lay.pack(wq.random_weights(lay, 4))
    s = np.abs(s) + np.float32(0.5)
    p = p * (lay.grad_mask() if kind != "inception" else 1.0)
    eng.set_params(p.astype(np.float32))
    eng.set_bn_state(s)
    if kind == "inception":
        eng.set_option("dropout_seed", 9)
    if prepare is not None:
        prepare(eng, lay)
    return lay, eng


def batches(n, seed=21):
    rng = np.random.default_rng(seed)
    return [(ec.synth_x(rng, B, T), (rng.random(B) < 0.5).astype(np.float32), rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32))
            for _ in range(n)]


def step(eng, batch, split=False):
    x, y, w = batch
    eng.set_batch(x)
    eng.set_targets(y, w)
    if split:   # the two-call form of a data-parallel step: gradient only, then Adam
        eng.train_step(B, LR, native.STEP_NO_APPLY)
        eng.apply_gradients(LR, 1.0)
    else:
        eng.train_step(B, LR)


def snapshot(eng):
    m, v, n = eng.get_opt_state()
    return (eng.get_params(), eng.get_bn_state(), m, v, np.int64(n), eng.get_grads())


def on(decay=DECAY, every=1, graphs=0):
    def prepare(eng, lay):
        eng.set_weight_ema(decay, every)
        if graphs:
            eng.set_option("graphs", 1)
    return prepare


def assert_ema(eng, want, updates, what=""):
    got, n = eng.get_ema_state()
    assert n == updates == eng.ema_updates(), (what, n, updates)
    if updates == 0:
        return   # (the vector has no meaning before the first update)
    if not same_bits(got, want):
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        raise AssertionError("%s: the average differs from the restatement at %d of %d parameters, first %d: %r vs %r"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


# ---------------------------------------------------------------------------------------------- 1. the EMA is the restatement
def check_restatement(lib, kind, every=1, split=False):
    lay, eng = start(lib, kind, on(every=every))
    ema, updates = None, 0
    for k, b in enumerate(batches(4)):
        step(eng, b, split)
        master = eng.get_params()
        before = updates
        ema, updates = averaging.ema_fold([master], DECAY, every, first_opt_step=k + 1, ema=ema, updates=updates)
        assert_ema(eng, ema, updates, "%s every %d after step %d" % (kind, every, k + 1))
        if before == 0 and updates == 1:
            assert same_bits(ema, master)   # the first update is a copy
    assert updates == 4 // every
    assert not same_bits(ema, eng.get_params())   # an average, not the iterate
    # a gradient-only step updates nothing, and neither does set_params
    x, y, w = batches(1, seed=5)[0]
    eng.set_batch(x)
    eng.set_targets(y, w)
    eng.train_step(B, LR, native.STEP_NO_APPLY)
    eng.set_params(eng.get_params() * np.float32(0.5))
    assert_ema(eng, ema, updates, "after a gradient-only step and set_params")
    eng.close()
    return eng.n_params


def check_non_finite_propagates(lib):
    """a non-finite master shows in the average, element by element; the restatement says the same"""
    lay, eng = start(lib, "block", on())
    bs = batches(2)
    step(eng, bs[0])
    p = eng.get_params()
    ema = averaging.ema_update(None, p, DECAY, 0)
    p[3], p[4], p[eng.n_params - 1] = np.inf, np.nan, -np.inf   # (the last element is in the scalar tail when P % 4 != 0)
    eng.set_params(p)
    eng.set_batch(bs[1][0])
    eng.set_targets(bs[1][1], np.zeros(B, np.float32))   # zero sample weights do not help: the forward is non-finite
    eng.train_step(B, LR)
    master = eng.get_params()
    want = averaging.ema_update(ema, master, DECAY, 1)
    got, n = eng.get_ema_state()
    assert n == 2 and same_bits(got, want)
    assert not np.all(np.isfinite(got))
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. observing only
def check_observing_only(lib, kind):
    runs = []
    for prepare in (None, on(), on(every=2)):
        lay, eng = start(lib, kind, prepare)
        outs = []
        for b in batches(4):
            step(eng, b)
            outs.append(eng.read_outputs(B)[0])
        runs.append((snapshot(eng), outs, eng))
    (plain, outs_p, _), (avg, outs_a, _), (avg2, outs_2, _) = runs
    assert all(np.all(np.isfinite(a)) for a in plain)
    assert all_same(plain, avg) and all_same(plain, avg2)   # parameters, BN state, Adam m / v / step, gradient
    assert all_same(outs_p, outs_a) and all_same(outs_p, outs_2)
    # without ema_forward the inference forward reads the master too
    x = batches(1, seed=8)[0][0]
    probs = []
    for _, _, eng in runs:
        eng.set_batch(x)
        eng.forward(B, training=False)
        probs.append(eng.read_outputs(B, want_loss=False)[0])
        assert same_bits(eng.get_forward_params(), eng.get_params())
        eng.close()
    assert all_same(probs[:1] * 2, probs[1:])


# ---------------------------------------------------------------------------------------------- 3. ema_forward
def eval_outputs(eng, x, y):
    """eval-mode probabilities and logits of x; the last batch's probabilities and the metric counters of a window evaluation
    in batches of 3"""
    eng.set_batch(x)
    eng.forward(B, training=False)
    p, z = eng.read_outputs(B, want_loss=False)[:2]
    eng.upload_store(0, x.reshape(-1))
    win = np.array([(0, 0, T, 0, i * T * 40) for i in range(B)], native.WINDOW_DTYPE)
    eng.metrics_reset()
    eng.evaluate_windows(win, y, 3)
    tail = eng.read_outputs(B - (B - 1) // 3 * 3, want_loss=False)[0]
    return p, z, tail, bytes(eng.metrics_raw())


def check_ema_forward(lib, kind):
    bs = batches(4)
    x, y, _ = batches(1, seed=8)[0]
    lay, eng = start(lib, kind, on())
    _, plain = start(lib, kind, on())   # the same calls in the same order, ema_forward never set: reads the master throughout
    eng.set_option("ema_forward", 1)
    # updates == 0: the master is read
    assert all_same(eval_outputs(eng, x, y), eval_outputs(plain, x, y))
    assert same_bits(eng.get_forward_params(), eng.get_params())
    for b in bs[:3]:
        step(eng, b)
        step(plain, b)
    ema, n = eng.get_ema_state()
    assert n == 3 and not same_bits(ema, eng.get_params())
    assert same_bits(eng.get_forward_params(), ema) and same_bits(plain.get_forward_params(), plain.get_params())
    # a twin whose master IS the average, with the same moving statistics
    _, twin = start(lib, kind)
    twin.set_params(ema)
    twin.set_bn_state(eng.get_bn_state())
    got, want, at_master = eval_outputs(eng, x, y), eval_outputs(twin, x, y), eval_outputs(plain, x, y)
    assert all_same(got, want)
    assert not same_bits(at_master[1], want[1])   # ... which is not what the master gives
    eng.set_option("ema_forward", 0)
    assert all_same(eval_outputs(eng, x, y), at_master)
    eng.set_option("ema_forward", 1)
    assert all_same(eval_outputs(eng, x, y), want)
    eval_outputs(plain, x, y), eval_outputs(plain, x, y)   # (call for call)
    # a training-mode forward reads the master
    for e in (eng, plain):
        e.set_batch(x)
        e.forward(B, training=True)
    assert same_bits(eng.read_outputs(B, want_loss=False)[1], plain.read_outputs(B, want_loss=False)[1])
    # ... and the option does not change the next train step: the master trajectory is the twin's
    step(eng, bs[3])
    step(plain, bs[3])
    assert all_same(snapshot(eng), snapshot(plain))
    assert all_same(eng.get_ema_state(), plain.get_ema_state())
    for e in (eng, twin, plain):
        e.close()


# ---------------------------------------------------------------------------------------------- 4. with weight_qat on
def check_with_weight_qat(lib, kind):
    bs = batches(4)
    x, y, _ = batches(1, seed=8)[0]

    def qat_on(eng, lay):
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)

    def both(eng, lay):
        qat_on(eng, lay)
        on()(eng, lay)
    lay, eng = start(lib, kind, both)
    _, never = start(lib, kind, both)      # never evaluates on the average
    for b in bs[:3]:
        step(eng, b)
        step(never, b)
    ema, _ = eng.get_ema_state()
    eng.set_option("ema_forward", 1)
    want = qat.forward_params_reference(lay, ema)
    assert same_bits(eng.get_forward_params(), want) and not same_bits(want, qat.forward_params_reference(lay, eng.get_params()))
    # the evaluation forward reads fake_quant(average): a twin whose master is the average, option on
    _, twin = start(lib, kind, qat_on)
    twin.set_params(ema)
    twin.set_bn_state(eng.get_bn_state())
    assert all_same(eval_outputs(eng, x, y), eval_outputs(twin, x, y))   # (the window evaluation leaves the shadow at the average)
    # the stale-shadow case: evaluate on the average -> train step -> evaluate on the master
    step(eng, bs[3])
    step(never, bs[3])
    assert all_same(snapshot(eng), snapshot(never))
    assert same_bits(eng.read_outputs(B)[1], never.read_outputs(B)[1])
    eng.set_option("ema_forward", 0)
    assert same_bits(eng.get_forward_params(), qat.forward_params_reference(lay, eng.get_params()))
    assert all_same(eval_outputs(eng, x, y), eval_outputs(never, x, y))
    assert all_same(eng.get_ema_state(), never.get_ema_state())
    for e in (eng, never, twin):
        e.close()


# ---------------------------------------------------------------------------------------------- 5. graph replay
def check_graph_replay(lib, kind="block"):
    bs = batches(6)
    finals = []
    for graphs in (0, 1):
        for every in (1, 2):
            lay, eng = start(lib, kind, on(every=every, graphs=graphs))
            for b in bs[:4]:
                step(eng, b)
            finals.append((snapshot(eng) + eng.get_ema_state(), eng))
    (e1, _), (e2, _), (g1, _), (g2, _) = finals
    assert all_same(e1, g1) and e1[-1] == g1[-1] == 4
    assert all_same(e2, g2) and e2[-1] == g2[-1] == 2
    assert not same_bits(e1[-2], e2[-2])
    for _, eng in finals:
        eng.close()
    # installing / removing the option between steps is honoured from the next step on
    lay, eng = start(lib, kind, on(graphs=1))
    _, ref = start(lib, kind)
    masters = []
    for k, b in enumerate(bs):
        if k == 2:
            eng.set_weight_ema(0.0)        # removed: steps 3 and 4 update nothing
            with pytest.raises(native.NativeError, match="error -1: .*no weight average"):
                eng.get_ema_state()
        if k == 4:
            eng.set_weight_ema(DECAY, 1)   # installed again: a new average, from step 5's master
        step(eng, b)
        step(ref, b)
        masters.append(eng.get_params())
        if k == 1:
            assert_ema(eng, averaging.ema_fold(masters, DECAY)[0], 2, "before the removal")
    assert all_same(snapshot(eng), snapshot(ref))
    assert_ema(eng, averaging.ema_fold(masters[4:], DECAY)[0], 2, "after the re-installation")
    eng.close()
    ref.close()


# ---------------------------------------------------------------------------------------------- 6. state round trip, refusals
def check_state_round_trip(lib, kind, every=1):
    bs = batches(4)
    lay, straight = start(lib, kind, on(every=every))
    for b in bs:
        step(straight, b)
    _, first = start(lib, kind, on(every=every))
    for b in bs[:2]:
        step(first, b)
    ema, updates = first.get_ema_state()
    m, v, n = first.get_opt_state()
    _, second = start(lib, kind, on(every=every))
    if kind == "inception":
        # the dropout generator's counter is no part of any saved state: the receiving context takes two steps of its own first,
        # so that its masks continue where `first`'s would; everything those steps left is overwritten below
        for b in batches(2, seed=77):
            step(second, b)
        second.set_weight_ema(DECAY, every)
    second.set_params(first.get_params())
    second.set_bn_state(first.get_bn_state())
    second.set_opt_state(m, v, n)
    second.set_ema_state(ema, updates)
    for b in bs[2:]:
        step(second, b)
    assert all_same(snapshot(straight), snapshot(second))
    a, b_ = straight.get_ema_state(), second.get_ema_state()
    assert same_bits(a[0], b_[0]) and a[1] == b_[1] == 4 // every
    for e in (straight, first, second):
        e.close()


def check_refusals(lib, kind):
    bs = batches(2)
    lay, fresh = start(lib, kind)
    step(fresh, bs[0])
    want = snapshot(fresh)
    fresh.close()

    def no(call, word):
        with pytest.raises(native.NativeError, match="error -1: .*" + word):
            call()
    lay, eng = start(lib, kind)
    P = eng.n_params
    for decay in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        no(lambda: eng.set_weight_ema(decay, 1), "decay")
    no(lambda: eng.set_weight_ema(0.9, 0), "every_steps")
    no(lambda: eng.set_weight_ema(0.9, -3), "every_steps")
    no(lambda: eng.set_option("ema_forward", 1), "weight average")   # none of them installed one
    no(lambda: eng.get_ema_state(), "weight average")
    no(lambda: eng.set_ema_state(np.zeros(P, np.float32), 1), "weight average")
    step(eng, bs[0])
    assert all_same(snapshot(eng), want)   # the context is usable: the step of a fresh context
    # with the option installed: refusals leave the average untouched
    eng.set_weight_ema(DECAY, 1)
    step(eng, bs[1])
    ema, n = eng.get_ema_state()
    assert n == 1 and same_bits(ema, eng.get_params())
    for decay, every, word in ((1.0, 1, "decay"), (-1.0, 1, "decay"), (0.5, 0, "every_steps")):
        no(lambda: eng.set_weight_ema(decay, every), word)
    no(lambda: eng.set_ema_state(np.zeros(P - 1, np.float32), 1), "size")
    no(lambda: eng.set_ema_state(np.zeros(P + 1, np.float32), 1), "size")
    no(lambda: eng.set_ema_state(np.zeros(P, np.float32), -1), "size")
    no(lambda: eng.nl.check(eng.nl.lib.mww_get_ema_state(eng.h, None, P - 1, None)), "size")
    no(lambda: eng.set_option("ema_forward", 2), "0 or 1")
    assert all_same(eng.get_ema_state(), (ema, n))
    eng.set_option("ema_forward", 1)
    eng.set_weight_ema(0.0)   # removing the average turns the option off with it
    assert same_bits(eng.get_forward_params(), eng.get_params())
    no(lambda: eng.set_option("ema_forward", 1), "weight average")
    eng.close()


# ---------------------------------------------------------------------------------------------- 7. the loop
FIRST_STEP = 3


def loop_config(tmp_path, name, averaging_map="default", **over):
    import int8_in_loop_checks as ilc
    import streaming_validation_checks as svc
    cfg = svc.config(tmp_path, name, ilc.SVQ, prefetch_batches=0, **over)
    if averaging_map == "default":
        averaging_map = dict(decay=DECAY, first_step=FIRST_STEP)
    if averaging_map is not None:
        cfg["weight_averaging"] = averaging_map
    return cfg


class Recorder:
    """records master and BN moving statistics behind every train step of every engine (by monkeypatching Engine.train_step)"""

    def __init__(self, monkeypatch):
        self.masters, self.states = [], []
        plain = native.Engine.train_step
        rec = self

        def train_step(eng, *a, **k):
            plain(eng, *a, **k)
            rec.masters.append(eng.get_params())
            rec.states.append(eng.get_bn_state())
        monkeypatch.setattr(native.Engine, "train_step", train_step)

    def clear(self):
        del self.masters[:], self.states[:]


def averaged_variables(lay, master, state, ema):
    vec = master.copy()
    trainable = lay.grad_mask() != 0
    vec[trainable] = ema[trainable]
    return lay.unpack(vec, state)


def arrays_of(path):
    with np.load(path + ".npz") as z:
        return [z[k].tobytes() for k in sorted(z.files)]


def summary_of(model):
    lines = []
    model.summary(print_fn=lines.append)
    return lines


def check_loop(lib, tmp_path, caplog, monkeypatch):
    import mining_checks as mc
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    from microwakeword_amd import mixednet
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    rec = Recorder(monkeypatch)
    cfg = loop_config(tmp_path, "avg")
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        model, _ = smc.run_loop(lib, cfg)
    said = [r.getMessage() for r in caplog.records if "weight averaging" in r.getMessage()]
    assert len(said) == 1 and said[0].startswith("Step #%d: weight averaging on" % FIRST_STEP), said
    assert [(e["step"], e["weight_averaging"]) for e in svc.log_of(cfg, "train")] == [(4, 1), (8, 1), (12, 1)]
    assert any("Weight averaging" in line and "0.9" in line for line in summary_of(model))
    assert len(rec.masters) == smc.STEPS
    lay = model.layout
    # the average at every step, by the restatement over the recorded masters (installed before step 3: its update is the copy)
    emas = {}
    ema, updates = None, 0
    for k in range(FIRST_STEP, smc.STEPS + 1):
        ema, updates = averaging.ema_fold([rec.masters[k - 1]], DECAY, 1, k, ema, updates)
        emas[k] = ema
    got, n = model.engine.get_ema_state()
    assert n == updates == smc.STEPS - FIRST_STEP + 1 and same_bits(got, ema)
    # what each boundary wrote is the averaged model of its step ...
    at = {}
    for k in svc.BOUNDARIES:
        at[k] = [w.tobytes() for w in averaged_variables(lay, rec.masters[k - 1], rec.states[k - 1], emas[k])]
        raw = [w.tobytes() for w in lay.unpack(rec.masters[k - 1], rec.states[k - 1])]
        assert at[k] != raw
        path = svc.weights_at(cfg, k) if k != smc.STEPS else os.path.join(cfg["train_dir"], "last_weights.weights.h5")
        assert arrays_of(path) == at[k], k
    assert arrays_of(svc.weights_at(cfg, smc.STEPS)) == at[smc.STEPS]
    # ... best_weights among them, the checkpoint the master of the last step, with the average beside the Adam state
    best = arrays_of(os.path.join(cfg["train_dir"], "best_weights.weights.h5"))
    assert best in list(at.values())
    ckpt = os.path.join(cfg["train_dir"], "restore", "ckpt")
    assert arrays_of(ckpt + ".weights") == [w.tobytes() for w in lay.unpack(rec.masters[-1], rec.states[-1])]
    assert [w.tobytes() for w in model.get_weights()] == arrays_of(ckpt + ".weights")   # outside the context: the master
    with np.load(ckpt + ".opt.npz") as z:
        assert same_bits(z["ema"], ema) and int(z["ema_updates"]) == updates and float(z["ema_decay"]) == DECAY and int(z["ema_every_steps"]) == 1
    # inside the context the model evaluates on and returns the average; BN statistics from the master model
    with model.averaged_weights():
        assert [w.tobytes() for w in model.get_weights()] == at[smc.STEPS]
        assert same_bits(model.engine.get_forward_params(), ema)
        with model.master_weights():
            assert [w.tobytes() for w in model.get_weights()] == arrays_of(ckpt + ".weights")
    assert same_bits(model.engine.get_forward_params(), rec.masters[-1])
    # stopped after step 8 and restored: the same average, master and files as the uninterrupted run
    cut = loop_config(tmp_path, "cut", training_steps=[6, 2])
    rec.clear()
    smc.run_loop(lib, cut)
    assert all_same(rec.masters, rec.masters[:8]) and len(rec.masters) == 8
    rest = dict(cut, training_steps=[4], learning_rates=[cfg["learning_rates"][1]])
    state = mc.rng_state()
    random.seed(1)   # the handler orders its sample lists on the global generators when it is made: as run_loop makes it ...
    np.random.seed(1)
    restored = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=99, max_batch=64)
    fh = FeatureHandler(rest, engine=restored.engine)
    random.setstate(state[0])   # ... and the draws go on where the stopped run left them
    np.random.set_state(state[1])
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        tr.train(restored, rest, fh, verbose=False)
    said = [r.getMessage() for r in caplog.records if "weight averaging" in r.getMessage()]
    assert len(said) == 1 and "continues from the checkpoint (6 updates" in said[0], said
    assert restored.engine.get_opt_state()[2] == smc.STEPS
    got, n = restored.engine.get_ema_state()
    assert n == updates and same_bits(got, ema)
    assert same_bits(restored.engine.get_params(), model.engine.get_params())
    for name in ("last_weights.weights.h5", os.path.join("restore", "ckpt.weights")):
        assert arrays_of(os.path.join(cut["train_dir"], name)) == arrays_of(os.path.join(cfg["train_dir"], name)), name
    with np.load(os.path.join(cut["train_dir"], "restore", "ckpt.opt.npz")) as a, np.load(ckpt + ".opt.npz") as b:
        assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)


def check_loop_without_the_key(lib, tmp_path):
    """no key: the files of a run in which the option never existed (a second run whose first_step lies beyond its last step
    never installs it); the train scalars carry no weight_averaging field and the optimizer state no average"""
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    cfg = loop_config(tmp_path, "plain", averaging_map=None)
    model, _ = smc.run_loop(lib, cfg)
    assert not getattr(model, "weight_averaging", None) and all("weight_averaging" not in e for e in svc.log_of(cfg, "train"))
    assert not any("Weight averaging" in line for line in summary_of(model))
    with pytest.raises(native.NativeError, match="no weight average"):
        model.engine.get_ema_state()
    with model.averaged_weights():   # a no-op
        assert same_bits(model.engine.get_forward_params(), model.engine.get_params())
    late = loop_config(tmp_path, "late", averaging_map=dict(decay=DECAY, first_step=smc.STEPS + 1))
    model_l, _ = smc.run_loop(lib, late)
    assert [e["weight_averaging"] for e in svc.log_of(late, "train")] == [0, 0, 0]
    names = ["last_weights.weights.h5", "best_weights.weights.h5", os.path.join("restore", "ckpt.weights")]
    names += [os.path.relpath(svc.weights_at(cfg, k), cfg["train_dir"]) for k in svc.BOUNDARIES[:-1]]
    for name in names:
        assert arrays_of(os.path.join(cfg["train_dir"], name)) == arrays_of(os.path.join(late["train_dir"], name)), name
    with np.load(os.path.join(cfg["train_dir"], "restore", "ckpt.opt.npz")) as a, np.load(os.path.join(late["train_dir"], "restore", "ckpt.opt.npz")) as b:
        assert sorted(a.files) == sorted(b.files) == ["lr", "m", "step", "v"] and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    # ... and an optimizer-state file written without the average still loads, into a model that has one or not
    model_l.load_optimizer_state(os.path.join(cfg["train_dir"], "restore", "ckpt.opt.npz"))
    assert not getattr(model_l, "weight_averaging", None)


BAD_MAPPINGS = ((dict(first_step=3), "decay"), (dict(decay=0.9), "first_step"), (dict(decay=0.0, first_step=3), "decay"),
                (dict(decay=1.0, first_step=3), "decay"), (dict(decay=-0.5, first_step=3), "decay"), (dict(decay="0.9", first_step=3), "decay"),
                (dict(decay=True, first_step=3), "decay"), (dict(decay=float("nan"), first_step=3), "decay"),
                (dict(decay=0.9, first_step=-1), "first_step"), (dict(decay=0.9, first_step=2.5), "first_step"),
                (dict(decay=0.9, first_step=True), "first_step"), (dict(decay=0.9, first_step=3, every_steps=0), "every_steps"),
                (dict(decay=0.9, first_step=3, every_steps=1.5), "every_steps"), (dict(decay=0.9, first_step=3, momentum=0.9), "momentum"),
                ([0.9, 3], "mapping"), (0.9, "mapping"))
