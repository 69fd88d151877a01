"""Call sequences that do not wait for the device, across the ring of mailboxes (csrc/mww_lib.hip: mail_begin / mail_commit, the
``hyper`` words the kernels read when they EXECUTE, descriptor-only batches, labels read in place from a mailbox's HBM copy, the
cache of captured steps), held to equality against the same calls made one at a time.

The twin method: a *script* - a seeded list of ABI calls - runs on two fresh engines that start from identical weights.
  * the pipelined twin has the options the product trains with ("fused_input" 1, "graphs" 0 or 1) and waits for nothing until
    the script ends (or where the script itself reads outputs);
  * the stepwise twin has "fused_input" 0, "graphs" 0 and synchronises after every call.
Gathered inputs are the same floats as materialised ones and a replayed graph runs the same kernels (engine_checks
check_fused_input, test_determinism), so parameters, BN state, Adam slots, metric counters, outputs and the batch read back must be
EQUAL, not close.  The two twins could still be wrong together; the Adam restatement below anchors the stepwise twin's optimizer
to float64 NumPy, and engine_checks holds its gradients to the float64 oracle.

Shared by tests/test_pipeline_gpu.py (MI355X) and tests/test_pipeline_emulated.py (tests/hipemu: launches run inline there, so
ordering cannot fail, but which slot is lazy, where the labels are, what the graph cache is keyed by is plain host logic)."""
import random

import numpy as np

import engine_checks as ec
from microwakeword_amd import native
from microwakeword_amd.data import FeatureHandler
from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout, MixedNetLayout
from oracle import model_oracle as mo

U = 2.0 ** -24   # float32 unit roundoff
RING = 8         # engine.hip.h kRing
POLICY = dict(time_mask_max_size=4, time_mask_count=2, freq_mask_max_size=4, freq_mask_count=2)
KINDS = {"mixednet": ("block", ec.DEF), "notebook": ("block", ec.NOTEBOOK), "inception": ("inception", ec.INC),
         "graph_mixednet": ("graph", ec.GRAPH_MIXEDNET)}


def lr_of(k):
    """a learning rate per step, all distinct: a step that reads another mailbox slot's hyper[0] changes bits"""
    return 1e-3 * (1.0 + k / 8.0)


_weights = {}


def initial_weights(kind, T):
    if (kind, T) not in _weights:
        family, flags = KINDS[kind]
        om = ec.perturbed_inception_oracle(T, flags) if family == "inception" else ec.perturbed_oracle(T, flags=flags)
        _weights[(kind, T)] = om.get_weights()
    return _weights[(kind, T)]


def open_engine(lib, kind, T, max_batch, pipelined, graphs=0):
    family, flags = KINDS[kind]
    lay = {"block": MixedNetLayout, "inception": InceptionLayout, "graph": GraphMixedNetLayout}[family](flags, T)
    eng = native.Engine(lib=lib, **lay.engine_args(max_batch))
    eng.set_grad_mask(lay.grad_mask())
    p, s = lay.pack(initial_weights(kind, T))
    eng.set_params(p)
    eng.set_bn_state(s)
    eng.set_option("fused_input", 1 if pipelined else 0)
    eng.set_option("graphs", graphs if pipelined else 0)
    if family == "inception":
        eng.set_option("dropout_seed", 1234)   # generated masks: the step's counter travels in hyper[2..3] of its mailbox
    return eng


class Twin:
    """One engine of a twin pair.  Calls that only enqueue go through here: the stepwise twin waits after each, the pipelined one
    counts the mailbox commits (mww_train_step, mww_forward, mww_apply_gradients: one each) made since the host last waited."""

    def __init__(self, eng, pipelined):
        self.eng, self.pipelined = eng, pipelined
        self.unwaited = self.most_unwaited = 0

    def _after(self, commits):
        if self.pipelined:
            self.unwaited += commits
            self.most_unwaited = max(self.most_unwaited, self.unwaited)
        else:
            self.eng.synchronize()

    def waited(self):   # after a call that synchronises the stream (any get_* / read_* / set_batch)
        self.unwaited = 0

    def set_targets(self, y, w):
        self.eng.set_targets(y, w)
        self._after(0)

    def assemble(self, win, masks, nt, nf):
        self.eng.assemble(win, masks, nt, nf)
        self._after(0)

    def next_batch(self, fh, B, T):
        fh.next_training_batch_on_device(B, T, "default", POLICY)
        self._after(0)

    def set_batch(self, x):
        self.eng.set_batch(x)
        self.waited()

    def train_step(self, B, lr, flags=0):
        self.eng.train_step(B, lr, flags=flags)
        self._after(1)

    def apply_gradients(self, lr, scale):
        self.eng.apply_gradients(lr, scale)
        self._after(1)

    def forward(self, B, training, update_metrics):
        self.eng.forward(B, training=training, update_metrics=update_metrics)
        self._after(1)

    def evaluate_windows(self, win, labels, batch):
        self.eng.evaluate_windows(win, labels, batch)
        self._after(-(-len(labels) // batch))

    def metrics_reset(self):
        self.eng.metrics_reset()
        self._after(0)

    def read_outputs(self, rows, want_loss):
        p, z, loss = self.eng.read_outputs(rows, want_loss=want_loss)
        self.waited()
        return dict(probs=p.copy(), logits=z.copy(), loss=np.float64(loss if want_loss else 0.0))


def raw_counters(eng):
    return np.frombuffer(bytes(eng.metrics_raw()), np.uint8).copy()


def final_state(tw, out_rows, batch_rows, want_loss):
    """everything the twins are compared on; the outputs first (the first host wait of a pipelined script)"""
    eng = tw.eng
    d = tw.read_outputs(out_rows, want_loss) if out_rows else {}
    m, v, step = eng.get_opt_state()
    d.update(params=eng.get_params(), bn_state=eng.get_bn_state(), adam_m=m, adam_v=v, step=np.int64(step), metrics=raw_counters(eng))
    if batch_rows:
        d["batch"] = eng.get_batch(batch_rows)
    return d


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        if a[k].dtype.kind == "f":   # (assert_array_equal takes two NaNs for equal: twins that both diverged must not pass)
            assert np.all(np.isfinite(a[k])) and np.all(np.isfinite(b[k])), "%s: %s is not finite" % (what, k)
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


# ------------------------------------------------------------------------------------------ Adam restatement (case 2)
class AdamRestatement:
    """Keras Adam in float64 NumPy on the ENGINE'S OWN gradients: m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2),
    p -= alpha m / (sqrt(v) + eps), alpha = lr sqrt(1 - b2^t) / (1 - b1^t), eps = 1e-7, lr the float32 the ABI takes, and b1, b2 the
    float32 constants 0.9f, 0.999f (Keras casts its betas to the variables' type; the decimal 0.999 has 1 - b2 216u away from
    1 - 0.999f, a shift that cancels between alpha and sqrt(v) only in a run that starts at t = 0, and only up to eps).
    Free running: it starts from the engine's state once and never looks at it again.

    Bound, from u = 2^-24 alone, per step and element, summed over the steps taken.
      m: float32 rounds (g - m), the product with (1 - b1) and the sum; |g - m| <= 2 max(|m|, |g|): <= 4u max(|m|, |g|).
      v: the same with g^2: <= 4u max(v, g^2).
      p: u |p| for the subtraction, 8u |update| for sqrtf, + eps, the quotient, the product and the three operations of alpha, and
         the cancellation inside alpha: adam_alpha (mww_lib.hip) forms 1 - powf(b, t) in float32; powf is good to one ulp = 2u b^t,
         which is 2u b^t / (1 - b^t) of the difference (1 - 0.999^2 = 0.002: 1000u).  Through the square root (b2) resp. the
         quotient (b1): (u b2^t / (1 - b2^t) + 2u b1^t / (1 - b1^t)) |update|.  Keras' float32 alpha has the same term.
         And, the restatement running free, what the engine's own m and v differ by enters its update: alpha dm / (sqrt(v) + eps)
         + |update| dsv / (sqrt(v) + eps), dsv = min(dv / sqrt(v), sqrt(dv)) the distance of the square roots.  dm and dv are the
         sums of the roundings above without the coarsening to a maximum, 2u (1 - b1) |g - m| + u |m'| and
         u (1 - b2) (g^2 + 2 |g^2 - v|) + u v' (where v' = 0.001 g^2 the maximum form would allow sqrt(v) 2000u)."""

    def __init__(self, eng):
        m, v, t = eng.get_opt_state()
        self.m, self.v, self.t = m.astype(np.float64), v.astype(np.float64), int(t)
        self.p = eng.get_params().astype(np.float64)
        self.em, self.ev, self.ep, self.dm, self.dv = (np.zeros_like(self.p) for _ in range(5))
        self.worst = dict(m=0.0, v=0.0, p=0.0)

    @staticmethod
    def _ratio(got, want, bound):
        d = np.abs(got.astype(np.float64) - want)
        if not np.all(np.isfinite(d)):
            return float("inf")
        r = np.divide(d, bound, out=np.where(d > 0, np.inf, 0.0), where=bound > 0)
        return float(r.max())

    def step(self, eng, lr, gscale=1.0):
        b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), 1e-7
        g = eng.get_grads().astype(np.float64) * gscale
        self.t += 1
        lr = float(np.float32(lr))
        b1p, b2p = b1 ** self.t, b2 ** self.t
        alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        self.em += 4 * U * np.maximum(np.abs(self.m), np.abs(g))
        self.ev += 4 * U * np.maximum(self.v, g * g)
        self.dm += 2 * U * (1.0 - b1) * np.abs(g - self.m)
        self.dv += U * (1.0 - b2) * (g * g + 2 * np.abs(g * g - self.v))
        self.m += (g - self.m) * (1.0 - b1)
        self.v += (g * g - self.v) * (1.0 - b2)
        self.dm += U * np.abs(self.m)
        self.dv += U * self.v
        sv = np.sqrt(self.v)
        upd = alpha * self.m / (sv + eps)
        self.p -= upd
        dsv = np.minimum(np.divide(self.dv, sv, out=np.full_like(sv, np.inf), where=sv > 0), np.sqrt(self.dv))
        self.ep += (U * np.abs(self.p) + (8 + b2p / (1.0 - b2p) + 2 * b1p / (1.0 - b1p)) * U * np.abs(upd)
                    + (alpha * self.dm + np.abs(upd) * dsv) / (sv + eps))
        m, v, t = eng.get_opt_state()
        assert t == self.t, (t, self.t)
        r = dict(m=self._ratio(m, self.m, self.em), v=self._ratio(v, self.v, self.ev), p=self._ratio(eng.get_params(), self.p, self.ep))
        for k in r:
            self.worst[k] = max(self.worst[k], r[k])
        return r


# ------------------------------------------------------------------------------------------ cases 1, 2, 5: train steps only
def run_lr_ring(lib, kind, T, B, steps, pipelined, graphs=0, depth=0, adam=False):
    random.seed(5)
    np.random.seed(5)
    eng = open_engine(lib, kind, T, B, pipelined, graphs)
    fh = None
    try:
        tw = Twin(eng, pipelined)
        fh = FeatureHandler(ec.learnable_config(T=T), engine=eng)
        fh.use_private_rng(prefetch=depth)
        ad = AdamRestatement(eng) if adam else None
        trace = []
        for k in range(steps):
            tw.next_batch(fh, B, T)
            tw.train_step(B, lr_of(k))
            if not pipelined:
                trace.append(tw.read_outputs(B, True))
            if ad:
                ad.step(eng, lr_of(k))
        unwaited = tw.unwaited
        out = final_state(tw, B, B, True)
        report = {}
        if ad:
            report["steps"] = dict(ad.worst)
            # gradients formed by one call, scaled and applied by another
            ad = AdamRestatement(eng)
            for k in range(steps, steps + 4):
                tw.next_batch(fh, B, T)
                tw.train_step(B, lr_of(k), flags=native.STEP_NO_APPLY)
                tw.apply_gradients(lr_of(k), 0.5)
                ad.step(eng, lr_of(k), gscale=0.5)
            report["apply_gradients"] = dict(ad.worst)
            # a long run's step count: 0.9^t underflows to 0 in float32, 0.999^t is 3.5e-44 (alpha = lr)
            m, v, _ = eng.get_opt_state()
            eng.set_opt_state(m, v, 100000)
            ad = AdamRestatement(eng)
            for k in range(steps + 4, steps + 8):
                tw.next_batch(fh, B, T)
                tw.train_step(B, lr_of(k))
                ad.step(eng, lr_of(k))
            assert eng.get_opt_state()[2] == 100004
            report["step_100000"] = dict(ad.worst)
        return dict(out=out, unwaited=unwaited, trace=trace, adam=report)
    finally:
        if fh is not None:
            fh._drop_prefetcher()
        eng.close()


_stepwise = {}


def stepwise_lr_ring(lib, kind, T, B, steps):
    """the stepwise twin of a train-steps-only script, computed once and shared (it also carries the Adam restatement)"""
    key = (id(lib), kind, T, B, steps)
    if key not in _stepwise:
        _stepwise[key] = run_lr_ring(lib, kind, T, B, steps, False, adam=(kind == "mixednet"))
    return _stepwise[key]


def check_lr_ring(lib, kind="mixednet", T=60, B=8, steps=26, graphs=0, depth=0):
    """Cases 1 and 5: `steps` train steps, a learning rate of its own each, nothing read until the end."""
    ref = stepwise_lr_ring(lib, kind, T, B, steps)
    got = run_lr_ring(lib, kind, T, B, steps, True, graphs, depth)
    # the script really wraps: that many commits with no host wait in between (the ring has 8 slots)
    assert got["unwaited"] == steps and steps >= 2 * RING + 2, (got["unwaited"], steps)
    assert ref["out"]["step"] == steps
    assert_same(ref["out"], got["out"], "%s graphs %d prefetch %d" % (kind, graphs, depth))
    np.testing.assert_array_equal(ref["trace"][-1]["probs"], got["out"]["probs"])


def check_adam_restatement(lib, T=60, B=8, steps=26):
    """Case 2: m, v and the parameters of the stepwise twin after every step against AdamRestatement, within its derived bound."""
    rep = stepwise_lr_ring(lib, "mixednet", T, B, steps)["adam"]
    print("Adam slots against the float64 restatement, worst |difference| / derived bound: %s" % rep)
    assert all(r[k] <= 1.0 for r in rep.values() for k in ("m", "v", "p")), rep
    return rep


# ------------------------------------------------------------------------------------------ case 3: mixed scripts
def eval_windows(fh, T, n, seed):
    win, labels, _ = fh._eval_windows("validation", T, "truncate_start")
    pick = np.random.default_rng(seed).permutation(win.shape[0])[:n]
    assert pick.size == n
    return win[pick], np.asarray(labels, np.float32)[pick]


def make_script(seed, T, Bmax, n_calls=60, reads=(19, 41)):
    """A seeded list of calls that keeps to the documented rules (a batch and targets of at least B rows before a step)."""
    rng = np.random.default_rng(9100 + seed)
    sizes = [Bmax, Bmax, Bmax, 3, 1]
    ops = ["batch_targets_first", "batch_targets_after", "prefetched", "set_batch", "step", "step", "step_twice", "no_apply_then_apply",
           "forward_eval", "forward_train", "targets", "evaluate_windows", "metrics_reset"]
    script, have_x, have_y, k = [], 0, 0, 0

    def targets(n):
        return (rng.random(n) < 0.5).astype(np.float32), rng.choice([0.5, 1.0, 2.0], size=n).astype(np.float32)

    while len(script) < n_calls:
        if len(script) in reads:
            script.append(("read",))
            continue
        op = ops[int(rng.integers(len(ops)))]
        B = min(have_x, have_y)
        if op in ("step", "step_twice", "no_apply_then_apply", "forward_eval", "forward_train") and B == 0:
            op = "batch_targets_first"
        if op in ("batch_targets_first", "batch_targets_after", "prefetched"):
            n = sizes[int(rng.integers(len(sizes)))]
            script.append((op, n))
            have_x = have_y = n
        elif op == "set_batch":
            n = sizes[int(rng.integers(len(sizes)))]
            script.append((op, ec.synth_x(rng, n, T), targets(n) if have_y < n else None))
            have_x, have_y = n, max(have_y, n)
        elif op == "targets":
            n = max(have_x, 1)
            script.append((op,) + targets(n))
            have_y = n
        elif op == "evaluate_windows":
            script.append((op, 3 * Bmax + 5, Bmax, int(rng.integers(1 << 30))))
            have_x = have_y = (3 * Bmax + 5) % Bmax or Bmax   # the rows of the call's last batch
        elif op == "metrics_reset":
            script.append((op,))
        elif op == "no_apply_then_apply":
            script.append((op, B, lr_of(k), float(rng.choice([1.0, 0.5]))))
            k += 1
        elif op == "step_twice":
            script.append((op, B, lr_of(k), lr_of(k + 1)))
            k += 2
        elif op == "step":
            script.append((op, B, lr_of(k)))
            k += 1
        else:
            script.append((op, B))
    return script


def make_revisit_script(T, Bmax, seed=0):
    """Not random: what a captured step bakes in besides its key.  (a) A second step on a batch whose mailbox slot has moved on,
    then, eight commits later, a new descriptor-only batch in the slot that second step ran in - three laps.  (b) A batch replaced
    through mww_set_batch while its labels still sit in the mailbox, then a step that reads no mailbox word (NO_APPLY: keyed by no
    slot) - three times, in three different slots, with other labels each time."""
    rng = np.random.default_rng(9300 + seed)
    script, k = [], 0
    for lap in range(3):
        script += [("batch_targets_first", Bmax), ("step_twice", Bmax, lr_of(k), lr_of(k + 1))]
        k += 2
        for i in range(RING - 1):
            script += [("prefetched" if i % 2 else "batch_targets_first", Bmax), ("step", Bmax, lr_of(k))]
            k += 1
    script.append(("read",))
    for rep in range(3):
        script += [("batch_targets_first", Bmax), ("set_batch", ec.synth_x(rng, Bmax, T), None), ("no_apply_then_apply", Bmax, lr_of(k), 0.5),
                   ("prefetched", Bmax), ("step", Bmax, lr_of(k + 1))]
        k += 2
    return script


def run_script(lib, script, kind, T, Bmax, pipelined, graphs):
    random.seed(6)
    np.random.seed(6)
    eng = open_engine(lib, kind, T, Bmax, pipelined, graphs)
    fh = None
    try:
        tw = Twin(eng, pipelined)
        fh = FeatureHandler(ec.learnable_config(T=T), engine=eng)
        fh.use_private_rng(prefetch=2)
        reads, trace = [], []
        out_rows, batch_rows, loss_valid = 0, 0, False
        for call in script:
            op = call[0]
            if op in ("batch_targets_first", "batch_targets_after"):
                d = fh.draw_training_batch(call[1], T, "default", POLICY)   # (on the launching thread; the streams continue)
                if op == "batch_targets_first":
                    tw.set_targets(d["labels"], d["weights"])
                tw.assemble(d["windows"], d["masks"], d["n_time"], d["n_freq"])
                if op == "batch_targets_after":
                    tw.set_targets(d["labels"], d["weights"])
                batch_rows = call[1]
            elif op == "prefetched":
                tw.next_batch(fh, call[1], T)
                assert fh._pf is not None
                batch_rows = call[1]
            elif op == "set_batch":
                if call[2] is not None:
                    tw.set_targets(*call[2])
                tw.set_batch(call[1])
                batch_rows = call[1].shape[0]
            elif op == "targets":
                tw.set_targets(call[1], call[2])
            elif op == "step":
                tw.train_step(call[1], call[2])
            elif op == "step_twice":
                tw.train_step(call[1], call[2])
                tw.train_step(call[1], call[3])
            elif op == "no_apply_then_apply":
                tw.train_step(call[1], call[2], flags=native.STEP_NO_APPLY)
                tw.apply_gradients(call[2], call[3])
            elif op == "forward_eval":
                tw.forward(call[1], False, True)
            elif op == "forward_train":
                tw.forward(call[1], True, False)
            elif op == "evaluate_windows":
                win, labels = eval_windows(fh, T, call[1], call[3])
                tw.evaluate_windows(win, labels, call[2])
                batch_rows = call[1] % call[2] or call[2]
            elif op == "metrics_reset":
                tw.metrics_reset()
            if op in ("step", "step_twice", "no_apply_then_apply", "forward_eval", "forward_train", "evaluate_windows"):
                out_rows = batch_rows if op == "evaluate_windows" else call[1]
                loss_valid = op in ("step", "step_twice", "no_apply_then_apply")
                if not pipelined:
                    trace.append(tw.read_outputs(out_rows, loss_valid))
            if op == "read" and out_rows:
                reads.append(tw.read_outputs(out_rows, loss_valid))
        out = final_state(tw, out_rows, batch_rows, loss_valid)
        return dict(out=out, reads=reads, trace=trace, most_unwaited=tw.most_unwaited)
    finally:
        if fh is not None:
            fh._drop_prefetcher()
        eng.close()


def check_mixed_script(lib, seed, kind="mixednet", T=60, Bmax=8, graphs=0, n_calls=60):
    """Case 3: every kind of call that touches the mailboxes, in a seeded order, batch sizes changing in between
    (`seed` "revisit": make_revisit_script)."""
    script = make_revisit_script(T, Bmax) if seed == "revisit" else make_script(seed, T, Bmax, n_calls)
    ref = run_script(lib, script, kind, T, Bmax, False, 0)
    got = run_script(lib, script, kind, T, Bmax, True, graphs)
    names = [c[0] for c in script]
    what = "%s seed %s graphs %d" % (kind, seed, graphs)
    assert len(ref["reads"]) == len(got["reads"])
    for i, (a, b) in enumerate(zip(ref["reads"], got["reads"])):
        assert_same(a, b, "%s, read %d" % (what, i))
    assert_same(ref["out"], got["out"], "%s (calls: %s)" % (what, names))
    return got["most_unwaited"]


# ------------------------------------------------------------------------------------------ case 4: evaluation across the ring
def check_evaluation_ring(lib, kind="mixednet", T=60, batch=4, full=19, rest=3):
    """mww_evaluate_windows: full + 1 forwards with no wait between them (2.5 laps of the ring at 19 * 4 + 3 windows) against the same
    windows sent a batch at a time with a wait and a read after each: identical raw counters; and the reference's metric
    definitions (oracle Metrics) applied to the read-back probabilities / logits give those counters exactly."""
    n = full * batch + rest
    cfg = ec.learnable_config(n=2 * n, T=T)
    results = []
    for pipelined in (True, False):
        random.seed(8)
        np.random.seed(8)
        eng = open_engine(lib, kind, T, batch, pipelined, 0)
        try:
            tw = Twin(eng, pipelined)
            fh = FeatureHandler(cfg, engine=eng)
            win, labels = eval_windows(fh, T, n, 17)
            tw.metrics_reset()
            outs = []
            if pipelined:
                tw.evaluate_windows(win, labels, batch)
                assert tw.unwaited == full + 1 and tw.unwaited >= 2 * RING + 2
            else:
                for s in range(0, n, batch):
                    b = min(batch, n - s)
                    tw.set_targets(labels[s:s + b], np.ones(b, np.float32))
                    tw.assemble(win[s:s + b], None, 0, 0)
                    tw.forward(b, False, True)
                    outs.append(tw.read_outputs(b, False))
            last = tw.read_outputs(rest, False)
            results.append(dict(last, metrics=raw_counters(eng), batch=eng.get_batch(rest)))
            m = native.metrics_from_raw(eng.metrics_raw())
        finally:
            eng.close()
    assert_same(results[1], results[0], "evaluate_windows against batch-at-a-time")
    exact = mo.Metrics()
    for s, o in zip(range(0, n, batch), outs):
        exact.update(o["probs"], labels[s:s + batch], o["logits"])
    e = exact.result()
    assert m["count"] == n
    for k in ("accuracy", "recall", "precision", "auc"):
        assert abs(m[k] - e[k]) < 1e-9, (k, m[k], e[k])
    for k in ("tp", "fp", "tn", "fn"):
        np.testing.assert_array_equal(m[k], e[k])


# ------------------------------------------------------------------------------------------ case 6: the training state is complete
def check_training_state_is_complete(lib, kind="mixednet", T=60, B=8, N=9, graphs=0):
    """params + BN state + (m, v, step) are the whole training state: N steps, the state carried into a fresh context, N more
    steps there = 2N steps in one context, bit for bit.  N is odd (the fresh context holds the other statistics hand-over parity
    than the uninterrupted run) and no multiple of 8 (another mailbox slot); the graph cache starts empty.  (Not for generated
    dropout: its counter is not part of the saved state.)"""
    assert N % 2 == 1 and N % RING != 0
    cfg = ec.learnable_config(T=T)
    batches = []

    def run(first, last, state=None):
        random.seed(7)
        np.random.seed(7)
        eng = open_engine(lib, kind, T, B, True, graphs)
        try:
            fh = FeatureHandler(cfg, engine=eng)   # (uploads the stores; every context holds them under the same ids)
            fh.use_private_rng(prefetch=0)
            while len(batches) < 2 * N:
                d = fh.draw_training_batch(B, T, "default", POLICY)
                batches.append({k: np.array(d[k]) for k in ("windows", "masks", "labels", "weights")} | dict(nt=d["n_time"], nf=d["n_freq"]))
            if state is not None:
                eng.set_params(state[0])
                eng.set_bn_state(state[1])
                eng.set_opt_state(*state[2])
            for k in range(first, last):
                d = batches[k]
                eng.set_targets(d["labels"], d["weights"])
                eng.assemble(d["windows"], d["masks"], d["nt"], d["nf"])
                eng.train_step(B, lr_of(k))
            m, v, step = eng.get_opt_state()
            return eng.get_params(), eng.get_bn_state(), (m, v, step)
        finally:
            eng.close()

    whole = run(0, 2 * N)
    half = run(0, N)
    resumed = run(N, 2 * N, state=half)
    assert whole[2][2] == resumed[2][2] == 2 * N
    for name, a, b in (("params", whole[0], resumed[0]), ("bn_state", whole[1], resumed[1]), ("adam m", whole[2][0], resumed[2][0]),
                       ("adam v", whole[2][1], resumed[2][1])):
        np.testing.assert_array_equal(a, b, err_msg="%s graphs %d: %s" % (kind, graphs, name))
    assert not np.array_equal(whole[0], half[0])
