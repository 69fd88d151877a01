"""What weight-only quantization-aware training costs and how far the shipped int8 weights sit from the trained grid
(DESIGN 11d).  Needs an MI355X.  Writes a report (default profiles/weight_qat.txt):

  * step cost: the default MixedNet train step at batch 1024 (194 frames, fixed batch resident in HBM), ``--steps`` steps
    enqueued back to back after ``--warmup`` steps and timed by a host clock around a stream synchronise; ``--reps``
    repetitions per arm, the arms alternating, each repetition in a fresh process; median and min..max per arm.  Arms: this
    tree with the option off, this tree with the option on, and - with ``--parent-tree DIR`` (a checkout of the parent commit
    with its library built) - the parent.  The off path's bar: no slower than the parent beyond the run-to-run spread.
  * off-grid share (a diagnostic, no bar): after a short QAT run on the synthetic set, per tensor the share of entries where
    the int8 weights ``quantize`` ships (BatchNorm folded) differ from the shadow's q up to the sign of the channel's gamma.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = dict(pointwise_filters="48, 48, 48, 48", residual_connection="0,0,0,0", repeat_in_block="1,1,1,1",
             mixconv_kernel_sizes="[5], [9], [13], [21]", max_pool=0, first_conv_filters=32, first_conv_kernel_size=3,
             spatial_attention=0, pooled=0, stride=1)
FRAMES = 194
LIB_NAME = "libmww_hip.so"


def time_steps(tree, qat_on, batch, steps, warmup):
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
    if qat_on:
        from microwakeword_amd import qat
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)
    for _ in range(warmup):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.train_step(batch, 1e-4)
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert np.all(np.isfinite(eng.get_params()))
    eng.close()
    print(json.dumps(dict(ms_per_step=ms)))


def step_cost(args, out):
    arms = [("off", ROOT, 0), ("on", ROOT, 1)]
    if args.parent_tree:
        arms.insert(0, ("parent", os.path.abspath(args.parent_tree), 0))
    times = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, tree, on in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, str(on), "--batch", str(args.batch), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("timing run %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
            times[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
    out.append("step cost: default MixedNet, batch %d, %d frames, %d steps back to back after %d warm-up steps, host clock around a stream "
               "synchronise;" % (args.batch, FRAMES, args.steps, args.warmup))
    out.append("           %d repetitions per arm, arms alternating, one process per repetition" % args.reps)
    med = {}
    for name, _, _ in arms:
        t = np.asarray(times[name])
        med[name] = float(np.median(t))
        out.append("  %-7s median %.4f ms/step   min %.4f   max %.4f   spread %.4f   (%s)" % (
            name, med[name], t.min(), t.max(), t.max() - t.min(), " ".join("%.4f" % v for v in t)))
    if "parent" in med:
        spread = max(np.ptp(times["parent"]), np.ptp(times["off"]))
        out.append("  off - parent = %+.4f ms/step (run-to-run spread %.4f): %s" % (
            med["off"] - med["parent"], spread, "within the spread" if med["off"] - med["parent"] <= spread else "SLOWER THAN THE SPREAD"))
    out.append("  on - off = %+.1f us/step (the refresh launch; DESIGN expects about 6 us for a tiny launch)" % ((med["on"] - med["off"]) * 1e3))
    return med


def off_grid(args, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import random
    import engine_checks as ec
    from microwakeword_amd import mixednet, qat, quantize
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    from microwakeword_amd.layout import _flag
    from microwakeword_amd.streaming import stream_description
    T, B, steps, first = 60, 16, args.qat_steps, args.qat_steps // 4
    with tempfile.TemporaryDirectory() as tmp:
        cfg = dict(ec.learnable_config(T=T), train_dir=os.path.join(tmp, "run"), summaries_dir=os.path.join(tmp, "run", "logs"), batch_size=B,
                   spectrogram_length=T, training_steps=[steps], learning_rates=[0.003], time_mask_max_size=[0], time_mask_count=[0],
                   freq_mask_max_size=[0], freq_mask_count=[0], positive_class_weight=[1.0], negative_class_weight=[1.0],
                   eval_step_interval=steps, target_minimization=0.9, minimization_metric=None, maximization_metric="accuracy",
                   weight_quantization_aware=dict(first_step=first))
        random.seed(1)
        np.random.seed(1)
        model = mixednet.model(FLAGS, (T, 40), B, seed=7, max_batch=64)
        tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
    weights = model.get_weights()
    lay = model.layout
    desc = stream_description(model.flags, lay.t_last, lay.frames, int(_flag(model.flags, "stride")), "stream")
    ranges = np.tile(np.float32([0.0, 26.0]), (len(quantize.tensor_names(desc)), 1))   # the int8 weights do not depend on the ranges
    shipped = quantize.quantize_weights(desc, weights, ranges).ops
    it = iter(np.asarray(w, np.float32) for w in weights)
    k1, c1 = int(desc["conv1_kernel"]), int(desc["conv1_filters"])
    rows = [("conv1", quantize.weight_params(next(it).reshape(k1 * 40, c1), 1)[0], np.ones(c1))]
    for kind, b, r, ks, ci, co in quantize.plan_ops(desc):
        if kind == "mix":
            rows.append(("b%d.mixconv" % b, quantize.weight_params(quantize.fold_mixconv(it, ks, ci)[0], 1)[0], np.ones(ci)))
        else:
            kern = next(it).reshape(ci, co)
            gamma = [next(it) for _ in range(4)][0]
            rows.append(("b%d.%s" % (b, "residual" if kind == "res" else "pointwise"), quantize.weight_params(kern, 1)[0], np.sign(gamma)))
    dense = next(it)
    rows.append(("dense", quantize.weight_params(dense.reshape(-1, 1), 1)[0].reshape(shipped[-1]["weights"].shape), np.ones(1)))
    out.append("off-grid share: default MixedNet, %d frames, batch %d, %d steps on the synthetic set with weight_quantization_aware first_step %d;"
               % (T, B, steps, first))
    out.append("                per tensor the share of int8 entries `quantize` ships (BN folded) that differ from the shadow's q x sign(gamma)")
    assert len(rows) == len(shipped)
    for (name, q, sign), op in zip(rows, shipped):
        want = q.astype(np.int32) * sign.astype(np.int32).reshape(1, -1)
        ship = op["weights"].astype(np.int32)
        assert ship.shape == want.shape, (name, ship.shape, want.shape)
        out.append("  %-14s %6d entries   off grid %.4f %%   (largest |difference| %d)" % (
            name, ship.size, 100.0 * float(np.mean(ship != want)), int(np.abs(ship - want).max())))
    fq = qat.fake_quant_weights(model, weights)
    moved = sum(int((a != b).sum()) for a, b in zip(weights, fq))
    out.append("  (the saved weights are the fp32 master: %d kernel entries differ from their grid value)" % moved)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", nargs=2, metavar=("TREE", "ON"), help=argparse.SUPPRESS)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--qat-steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_qat.txt"))
    args = ap.parse_args()
    if args.child:
        return time_steps(args.child[0], int(args.child[1]), args.batch, args.steps, args.warmup)
    out = ["weight-only quantization-aware training: step cost and off-grid share (tools/weight_qat_cost.py)",
           time.strftime("session %Y-%m-%d %H:%M:%S UTC", time.gmtime()), ""]
    step_cost(args, out)
    out.append("")
    off_grid(args, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
