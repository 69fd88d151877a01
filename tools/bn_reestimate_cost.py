"""What BatchNorm re-estimation for the weight average costs.  Needs an MI355X.  Writes a report (default
profiles/bn_reestimate.txt), with the protocol of tools/weight_ema_cost.py:

  * the default MixedNet train step at batch 1024 (194 frames, fixed batch resident in HBM), ``--steps`` steps enqueued back to
    back after ``--warmup`` steps and timed by a host clock around a stream synchronise; ``--reps`` repetitions per arm, the
    arms alternating, each repetition in a fresh process; median and min..max per arm.  Arms: with ``--parent-tree DIR`` (a
    checkout of the parent commit with its library built) the parent; this tree, which a configuration without the
    ``bn_reestimate`` key runs.  The bar: no slower than the parent by more than the parent's own run-to-run spread.
  * the product train loop on the synthetic benchmark stores (tools/train_loop_throughput.py's set-up: 200 steps of batch 1024,
    five boundaries, float streaming validation) with ``weight_averaging: {bn_reestimate: {samples: 4096}}``: the wall time of
    one pass (four batches of 1024; a stream synchronise on either side) next to that session's ``validate_streaming``.  No
    bar: recorded.
  * a diagnostic only: the validation loss of the averaged model behind that run with and without the pass.

Whether re-estimation improves validation on real data is not measured here.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import weight_ema_cost as wec   # noqa: E402  (the step-timing child and its shapes)

SAMPLES, DECAY = 4096, 0.99


def boundary_cost(batch, steps, samples):
    """(child process) the train loop with the key: ms of every pass and of every streaming validation, and the diagnostic"""
    sys.path.insert(0, ROOT)
    from microwakeword_amd import mixednet, streaming, synthetic
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    from microwakeword_amd.model import Model
    timed = {"reestimate_bn": [], "validate_streaming": []}
    plain_pass, plain_val = Model.reestimate_bn, streaming.validate_streaming

    def reestimate_bn(model, windows, b):
        model.engine.synchronize()
        t0 = time.perf_counter()
        plain_pass(model, windows, b)
        model.engine.synchronize()
        timed["reestimate_bn"].append(time.perf_counter() - t0)

    def validate_streaming(*a, **k):
        t0 = time.perf_counter()
        out = plain_val(*a, **k)
        timed["validate_streaming"].append(time.perf_counter() - t0)
        return out
    Model.reestimate_bn = reestimate_bn
    streaming.validate_streaming = validate_streaming
    cfg, _ = synthetic.benchmark_config(4096, 1234, n_val=256, n_ambient=32)
    d = tempfile.mkdtemp(prefix="mww_bnre_")
    cfg = dict(cfg, train_dir=d, summaries_dir=d + "/logs", batch_size=batch, spectrogram_length=wec.FRAMES, training_steps=[steps],
               learning_rates=[1e-3], time_mask_max_size=[5], time_mask_count=[2], freq_mask_max_size=[5], freq_mask_count=[2],
               positive_class_weight=[1.0], negative_class_weight=[1.0], eval_step_interval=max(1, steps // 5), target_minimization=0.9,
               minimization_metric=None, maximization_metric="accuracy", streaming_validation=dict(target_faph=0.5),
               weight_averaging=dict(decay=DECAY, first_step=1, bn_reestimate=dict(samples=samples, seed=0)))
    random.seed(0)
    np.random.seed(0)
    model = mixednet.model(synthetic.DEFAULT_MIXEDNET_FLAGS, (wec.FRAMES, 40), batch, seed=42, max_batch=batch)
    fh = FeatureHandler(cfg, engine=model.engine)
    tr.train(model, cfg, fh, verbose=False)
    losses = {}
    with model.averaged_weights():
        assert model.engine.ema_bn_valid()
        losses["with the pass"] = float(tr.validate_nonstreaming(cfg, fh, model, "validation")["loss"])
        model.engine.set_ema_state(*model.engine.get_ema_state())   # (clears the flag: the master's moving statistics again)
        assert not model.engine.ema_bn_valid()
        losses["without"] = float(tr.validate_nonstreaming(cfg, fh, model, "validation")["loss"])
    losses["the raw iterate"] = float(tr.validate_nonstreaming(cfg, fh, model, "validation")["loss"])
    model.engine.close()
    print(json.dumps(dict(timed={k: [1e3 * t for t in v] for k, v in timed.items()}, losses=losses)))


def run_child(argv, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("child %r failed (%d): %s" % (argv, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", nargs=2, metavar=("TREE", "EVERY"), help=argparse.SUPPRESS)
    ap.add_argument("--boundary-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_reestimate.txt"))
    args = ap.parse_args()
    if args.child:
        return wec.time_steps(args.child[0], int(args.child[1]), args.batch, args.steps, args.warmup)
    if args.boundary_child:
        return boundary_cost(args.batch, args.steps, args.samples)
    out = ["BatchNorm re-estimation for the weight average: cost (tools/bn_reestimate_cost.py)",
           time.strftime("session %Y-%m-%d %H:%M:%S UTC", time.gmtime()), ""]
    arms = [("absent", ROOT)]
    if args.parent_tree:
        arms.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    times = {name: [] for name, _ in arms}
    params = 0
    for _ in range(args.reps):
        for name, tree in arms:
            res = run_child(["--child", tree, "0", "--batch", str(args.batch), "--steps", str(args.steps), "--warmup", str(args.warmup)], 300)
            times[name].append(res["ms_per_step"])
            params = res["params"]
    out.append("step cost: default MixedNet (%d parameters), batch %d, %d frames, %d steps back to back after %d warm-up steps, host clock "
               "around a stream synchronise;" % (params, args.batch, wec.FRAMES, args.steps, args.warmup))
    out.append("           %d repetitions per arm, arms alternating, one process per repetition; no average installed" % args.reps)
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
    res = run_child(["--boundary-child", "--batch", str(args.batch), "--steps", str(args.steps), "--samples", str(args.samples)])
    out.append("")
    out.append("boundary: train.train on the synthetic benchmark stores, %d steps of batch %d, five boundaries, float streaming validation,"
               % (args.steps, args.batch))
    out.append("          weight_averaging {decay %g, first_step 1, bn_reestimate {samples %d}}: %d batches of %d per pass; wall time, a stream"
               % (DECAY, args.samples, args.samples // args.batch, args.batch))
    out.append("          synchronise on either side of a pass")
    for name in ("reestimate_bn", "validate_streaming"):
        v = res["timed"][name]
        out.append("  %-19s %s ms   (median after the first: %.2f ms)" % (name, ", ".join("%.2f" % t for t in v), float(np.median(v[1:]))))
    out.append("  (recorded, no bar)")
    out.append("")
    out.append("diagnostic only (synthetic data, %d steps): validation loss of the averaged model with the pass %.6f, without %.6f; of the raw "
               "iterate %.6f" % (args.steps, res["losses"]["with the pass"], res["losses"]["without"], res["losses"]["the raw iterate"]))
    out.append("Whether re-estimation improves validation on real data is not measured.")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
