"""What weight averaging costs in the train step.  Needs an MI355X.  Writes a report (default
profiles/weight_ema.txt):

  * the default MixedNet train step at batch 1024 (194 frames, fixed batch resident in HBM), ``--steps`` steps enqueued back to
    back after ``--warmup`` steps and timed by a host clock around a stream synchronise; ``--reps`` repetitions per arm, the
    arms alternating, each repetition in a fresh process; median and min..max per arm.
  * arms: with ``--parent-tree DIR`` (a checkout of the parent commit with its library built) the parent; this tree with no
    average installed (what a configuration without the ``weight_averaging`` key runs); this tree with the average on at
    ``every_steps`` 1 and 10.
  * the bar of the absent-key arm: no slower than the parent by more than the parent's own run-to-run spread of this session.
    The cost with the average on has no bar: it is recorded (DESIGN's working figure for one more tiny launch is about 6 us).

Whether averaging improves validation on real data is not measured here.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = dict(pointwise_filters="48, 48, 48, 48", residual_connection="0,0,0,0", repeat_in_block="1,1,1,1",
             mixconv_kernel_sizes="[5], [9], [13], [21]", max_pool=0, first_conv_filters=32, first_conv_kernel_size=3,
             spatial_attention=0, pooled=0, stride=1)
FRAMES = 194
LIB_NAME = "libmww_hip.so"
DECAY = 0.999


def time_steps(tree, every, batch, steps, warmup):
    """(child process) ms per step of the package in ``tree``; ``every`` 0 = no average installed"""
    sys.path.insert(0, tree)
    from microwakeword_amd import native
    from microwakeword_amd.layout import MixedNetLayout
    from microwakeword_amd.model import initial_weights
    nl = native.NativeLib(os.path.join(tree, "microwakeword_amd", LIB_NAME))
    if nl.device_count() < 1:
        raise RuntimeError("no GPU visible")
    lay = MixedNetLayout(FLAGS, FRAMES)
    eng = native.Engine(lib=nl, **lay.engine_args(batch))
    eng.set_grad_mask(lay.grad_mask())
    p, s = lay.pack(initial_weights(lay, 3))
    eng.set_params(p)
    eng.set_bn_state(s)
    rng = np.random.default_rng(0)
    eng.set_batch((rng.integers(0, 667, size=(batch, FRAMES, 40)).astype(np.float32) * np.float32(0.0390625)))
    eng.set_targets((rng.random(batch) < 0.5).astype(np.float32), np.ones(batch, np.float32))
    if every:
        eng.set_weight_ema(DECAY, every)
    for _ in range(warmup):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert np.all(np.isfinite(eng.get_params()))
    updates = -1
    if every:
        ema, updates = eng.get_ema_state()
        assert updates == (warmup + steps) // every and np.all(np.isfinite(ema))
    eng.close()
    print(json.dumps(dict(ms_per_step=ms, params=int(lay.n_params), updates=updates)))


def step_cost(args, out):
    arms = [("absent", ROOT, 0), ("every1", ROOT, 1), ("every10", ROOT, 10)]
    if args.parent_tree:
        arms.insert(0, ("parent", os.path.abspath(args.parent_tree), 0))
    times = {name: [] for name, _, _ in arms}
    params = 0
    for _ in range(args.reps):
        for name, tree, every in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, str(every), "--batch", str(args.batch), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("timing run %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
            res = json.loads(r.stdout.strip().splitlines()[-1])
            times[name].append(res["ms_per_step"])
            params = res["params"]
    out.append("step cost: default MixedNet (%d parameters), batch %d, %d frames, %d steps back to back after %d warm-up steps, host clock "
               "around a stream synchronise;" % (params, args.batch, FRAMES, args.steps, args.warmup))
    out.append("           %d repetitions per arm, arms alternating, one process per repetition; decay %g" % (args.reps, DECAY))
    med = {}
    for name, _, _ in arms:
        t = np.asarray(times[name])
        med[name] = float(np.median(t))
        out.append("  %-8s median %.4f ms/step   min %.4f   max %.4f   spread %.4f   (%s)" % (
            name, med[name], t.min(), t.max(), t.max() - t.min(), " ".join("%.4f" % v for v in t)))
    if "parent" in med:
        spread = float(np.ptp(times["parent"]))
        d = med["absent"] - med["parent"]
        out.append("  absent - parent = %+.4f ms/step (the parent's own run-to-run spread %.4f): %s" % (
            d, spread, "no slower than the parent beyond its spread" if d <= spread else "SLOWER THAN THE PARENT'S SPREAD"))
    for name in ("every1", "every10"):
        out.append("  %-7s - absent = %+.1f us/step (recorded, no bar; one more tiny launch is expected to cost about 6 us when it runs)"
                   % (name, (med[name] - med["absent"]) * 1e3))
    return med


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", nargs=2, metavar=("TREE", "EVERY"), help=argparse.SUPPRESS)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_ema.txt"))
    args = ap.parse_args()
    if args.child:
        return time_steps(args.child[0], int(args.child[1]), args.batch, args.steps, args.warmup)
    out = ["weight averaging: step cost (tools/weight_ema_cost.py)", time.strftime("session %Y-%m-%d %H:%M:%S UTC", time.gmtime()), ""]
    step_cost(args, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
