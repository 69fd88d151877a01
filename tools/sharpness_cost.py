"""What sharpness-aware steps and global-norm gradient clipping cost in the train step.  Needs an MI355X.  Writes a
report (default profiles/sharpness_aware.txt):

  * the default MixedNet train step at batch 1024 (194 frames, fixed batch resident in HBM), ``--steps`` steps enqueued back to
    back after ``--warmup`` steps and timed by a host clock around a stream synchronise; ``--reps`` repetitions per arm, the
    arms alternating, each repetition in a fresh process; median and min..max per arm.
  * arms: with ``--parent-tree DIR`` (a checkout of the parent commit with its library built) the parent; this tree with neither
    feature installed (what a configuration without the keys runs); clipping alone; the sharpness-aware step; both.
  * the bar of the absent-keys arm: no slower than the parent by more than the parent's own run-to-run spread of this session.
    The on-path costs have no bar: they are recorded against the absent-keys arm.

Whether sharpness-aware training narrows the float / int8 gap on real data is not measured here.
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
RHO, CLIP = 0.05, 1.0
ARMS = {"absent": (0.0, 0.0), "clip": (0.0, CLIP), "sam": (RHO, 0.0), "sam+clip": (RHO, CLIP)}


def time_steps(tree, arm, batch, steps, warmup):
    """(child process) ms per step of the package in ``tree``"""
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
    rho, clip = ARMS[arm]
    if rho:
        eng.set_sharpness_aware(rho)
    if clip:
        eng.set_grad_clip(clip)
    for _ in range(warmup):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert np.all(np.isfinite(eng.get_params()))
    norms = eng.get_grad_norms() if (rho or clip) else (0.0, 0.0)
    assert np.all(np.isfinite(norms))
    eng.close()
    print(json.dumps(dict(ms_per_step=ms, params=int(lay.n_params), first_norm=float(np.sqrt(norms[0])), final_norm=float(np.sqrt(norms[1])))))


def step_cost(args, out):
    arms = [(name, ROOT) for name in ARMS]
    if args.parent_tree:
        arms.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    times = {name: [] for name, _ in arms}
    last = {}
    for _ in range(args.reps):
        for name, tree in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "absent" if name == "parent" else name, "--batch", str(args.batch),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("timing run %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
            last[name] = json.loads(r.stdout.strip().splitlines()[-1])
            times[name].append(last[name]["ms_per_step"])
    out.append("step cost: default MixedNet (%d parameters), batch %d, %d frames, %d steps back to back after %d warm-up steps, host clock "
               "around a stream synchronise;" % (last["absent"]["params"], args.batch, FRAMES, args.steps, args.warmup))
    out.append("           %d repetitions per arm, arms alternating, one process per repetition; rho %g, clipping threshold %g" % (args.reps, RHO, CLIP))
    med = {}
    for name, _ in arms:
        t = np.asarray(times[name])
        med[name] = float(np.median(t))
        out.append("  %-8s median %.4f ms/step   min %.4f   max %.4f   spread %.4f   (%s)" % (
            name, med[name], t.min(), t.max(), t.max() - t.min(), " ".join("%.4f" % v for v in t)))
    if "parent" in med:
        spread = float(np.ptp(times["parent"]))
        d = med["absent"] - med["parent"]
        out.append("  absent - parent = %+.4f ms/step (the parent's own run-to-run spread %.4f): %s" % (
            d, spread, "no slower than the parent beyond its spread" if d <= spread else "SLOWER THAN THE PARENT'S SPREAD"))
    for name in ("clip", "sam", "sam+clip"):
        out.append("  %-8s - absent = %+.1f us/step = x %.3f (recorded, no bar); last step's gradient norms: first pass %.4g, consumed %.4g"
                   % (name, (med[name] - med["absent"]) * 1e3, med[name] / med["absent"], last[name]["first_norm"], last[name]["final_norm"]))
    return med


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", nargs=2, metavar=("TREE", "ARM"), help=argparse.SUPPRESS)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharpness_aware.txt"))
    args = ap.parse_args()
    if args.child:
        return time_steps(args.child[0], args.child[1], args.batch, args.steps, args.warmup)
    out = ["sharpness-aware steps and gradient clipping: step cost (tools/sharpness_cost.py)", time.strftime("session %Y-%m-%d %H:%M:%S UTC", time.gmtime()), ""]
    step_cost(args, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
