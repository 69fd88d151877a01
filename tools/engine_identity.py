"""Bit identity of the training engines between two builds of the library: a fixed, seeded list of cases, one JSON line per
case with the sha256 of what a context hands back - parameters, Adam state, BN state and gradients after three train steps,
the probabilities / logits / loss / metric counters of those steps and of one inference forward, the counters of
mww_evaluate_windows, the p1 / g1 / bn1 tensors of mww_debug_read, and (`sequence`) the outputs and parameters of a
training-mode forward followed by further train steps, which leaves the accumulator parities of the statistics hand-over out of
step with each other and, under "graphs", ends on a replayed graph.  For the cases that ask for it, `profile` is the sha256 of
the launch NAMES one more step records under option "profile" (no times).  The cases that install a step feature also hash what
that feature hands back (`fwd_params`: mww_get_forward_params, `ema`: mww_get_ema_state, `ema_bn`: mww_get_ema_bn_state, `norms`:
mww_get_grad_norms), after the three steps and again at the end.  The kernels sum in a fixed order, so a change that moves no
arithmetic leaves every hash as it was.

    python tools/engine_identity.py --lib A.so > a.jsonl      # every case
    python tools/engine_identity.py --lib B.so > b.jsonl
    python tools/engine_identity.py --compare a.jsonl b.jsonl  # two columns, exit status 1 when a hash differs
    python tools/engine_identity.py --lib tests/hipemu/libmww_emu.so --emulator   # the same list at emulator sizes

The cases: the default MixedNet under every schedule option of either owner, the notebook topology, the default Inception
under the graph engine's options, the Inception variant (two stem layers, dilation, sub-spectral groups, dropout), MixedNet
flag sets on the graph engine - generated dropout, residual branches, the attention / pooled heads, no first convolution,
captured graphs - both engines behind a world-1 pass-through exchange hook (sync-BN + gradient exchange), and the two-bucket
gradient exchange - and the step features on the default MixedNet (block engine) and on a MixedNet of the graph engine: a
"weight_qat" map, a weight average (every second step; "ema_forward" for the inference forward and the evaluation), a BatchNorm
re-estimation pass in front of that evaluation, sharpness-aware steps, clipping, both, and QAT + the average in a captured
step.  Batches come from a feature store through mww_assemble_batch (descriptor-only where the model gathers).
No oracle is consulted: this compares builds.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FIELDS = ("params", "adam", "bn_state", "grads", "outputs", "metrics", "forward", "evaluate", "debug", "sequence", "profile",
          "fwd_params", "ema", "ema_bn", "norms")
# step features a case installs -> the fields only such a case has ("-" elsewhere, like `profile`)
FEATURE_FIELDS = {"weight_qat": ("fwd_params",), "weight_ema": ("fwd_params", "ema", "ema_bn"), "bn_reestimate": ("fwd_params", "ema", "ema_bn"),
                  "sharpness_aware": ("norms",), "grad_clip": ("norms",)}
FEATURE_CASES = (("weight_qat", {}), ("weight_ema", {}), ("bn_reestimate", {}), ("sharpness_aware", {}), ("grad_clip", {}),
                 ("sharpness_aware+grad_clip", {}), ("weight_qat+weight_ema", {"graphs": 1}))
STEPS = 3
# train steps of `sequence`: one - or, under "graphs", one more than the mailbox ring has slots (kRing = 8), since a captured step
# is replayed only when mailbox slot and accumulator parities recur
SEQUENCE_STEPS, SEQUENCE_STEPS_GRAPHS = 1, 9
MIXEDNET_OPTIONS = ({}, {"bn_inline": 0}, {"tail_roles": 0}, {"side_stream": 1}, {"graphs": 1}, {"fused_input": 0}, {"bwd_wide": 0},
                    {"conv1_x6": 0}, {"conv1_x6_fwd": 1}, {"bwd_first_wide": 1}, {"dp_commit_late": 0}, {"dp_commit_late": 1},
                    {"pointwise_bf16": 1}, {"storage_bf16": 1})
INCEPTION_OPTIONS = ({}, {"graph_planar": 0}, {"graph_static_shapes": 0}, {"graph_role_split": 0}, {"profile_split": 1},
                     {"graph_frame_chunks": 2}, {"grid_graph": 64}, {"bn_inline": 0})


def cases(emulator):
    """(name, kind, flags, B, T, options, hook[, profile[, features]]) - hook: None or (sync_bn, reduce_grads); profile: hash the
    launch names; features: "+"-joined keys of FEATURE_FIELDS"""
    import engine_checks as ec
    mix = (4, 60) if emulator else (6, 194)
    note = (3, 204) if emulator else (6, 204)   # (first-conv stride 3: the shortest length the emulator tests run)
    inc = (4, 120) if emulator else (4, 150)
    tag = lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "defaults"   # noqa: E731
    out = [("mixednet/" + tag(o), "mixednet", ec.DEF, mix[0], mix[1], o, None) for o in MIXEDNET_OPTIONS]
    out.append(("notebook/defaults", "mixednet", ec.NOTEBOOK, note[0], note[1], {}, None))
    for o in INCEPTION_OPTIONS:
        if emulator and "grid_graph" in o:
            o = {"grid_graph": 8}   # (the emulated device has 4 CUs: at most 16 workgroups)
        out.append(("inception/" + tag(o), "inception", ec.INC, inc[0], inc[1], o, None))
    out.append(("inception/graphs=1", "inception", ec.INC, inc[0], inc[1], {"graphs": 1}, None))
    out.append(("inception/profile", "inception", ec.INC, inc[0], inc[1], {}, None, True))
    out.append(("inception/variant", "inception", ec.INC_VARIANT, inc[0], inc[1], {"dropout_seed": 77}, None))
    out.append(("graph_mixednet/dropout", "graph_mixednet", dict(ec.GRAPH_MIXEDNET, dropout=0.25), 3, 100, {"dropout_seed": 1234}, None))
    gmix = (3, 100) if emulator else (6, 150)
    for name, flags, o, prof in (("graphs=1", ec.GRAPH_MIXEDNET, {"graphs": 1}, False), ("profile", ec.GRAPH_MIXEDNET, {}, True),
                                 ("residual", ec.GRAPH_MIXEDNET_RESIDUAL, {}, False), ("full", ec.GRAPH_MIXEDNET_FULL, {}, False),
                                 ("attention", ec.GRAPH_MIXEDNET_HEADS[0], {}, False), ("noconv1", ec.GRAPH_MIXEDNET_NOCONV1, {}, False)):
        out.append(("graph_mixednet/" + name, "graph_mixednet", flags, gmix[0], gmix[1], o, None, prof))
    out.append(("mixednet/hook", "mixednet", ec.DEF, mix[0], mix[1], {}, (True, True)))
    out.append(("inception/hook", "inception", ec.INC, inc[0], inc[1], {}, (True, True)))
    out.append(("mixednet/grad_buckets=2", "mixednet", ec.DEF, mix[0], mix[1], {"grad_buckets": 2}, (False, True)))
    for kind, flags, (B, T) in (("mixednet", ec.DEF, mix), ("graph_mixednet", ec.GRAPH_MIXEDNET, gmix)):
        for feats, o in FEATURE_CASES:
            out.append(("%s/%s%s" % (kind, feats, "," + tag(o) if o else ""), kind, flags, B, T, o, None, False, feats))
    return out


def run_case(lib, name, kind, flags, B, T, options, hook, profile=False, features=""):
    from microwakeword_amd import native, qat
    from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout, MixedNetLayout
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    lay = {"mixednet": MixedNetLayout, "inception": InceptionLayout, "graph_mixednet": GraphMixedNetLayout}[kind](flags, T)
    eng = native.Engine(lib=lib, **lay.engine_args(B))
    if hasattr(lay, "grad_mask"):
        eng.set_grad_mask(lay.grad_mask())
    eng.set_params(rng.normal(0.0, 0.2, eng.n_params).astype(np.float32))
    if hook:
        eng.set_allreduce_hook(lambda ptr, n, fl: None, world_size=1, sync_bn=hook[0], reduce_grads=hook[1])
    feats = set(features.split("+")) if features else set()
    if "weight_qat" in feats:
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)
    if feats & {"weight_ema", "bn_reestimate"}:
        eng.set_weight_ema(0.9, every_steps=2)
    if "sharpness_aware" in feats:
        eng.set_sharpness_aware(0.05)
    if "grad_clip" in feats:
        eng.set_grad_clip(0.1)
    for k, v in options.items():
        eng.set_option(k, v)
    n_win = (STEPS + 1) * B + 2 * B + 1   # train steps, the inference forward, an evaluation of two batches and a part
    store = rng.integers(0, 667, size=((n_win + 1) * T, 40)).astype(np.uint16)
    eng.upload_store(0, store)
    win = np.zeros(n_win, native.WINDOW_DTYPE)
    for j in range(n_win):   # every third window starts with padding rows
        pad = (j % 3 == 2) * (5 + j % 7)
        win[j] = (0, pad, T - pad, 0, (j * T + j % 11) * 40)
    masks = np.stack([rng.integers(0, 30, size=(n_win, 4)), rng.integers(1, 5, size=(n_win, 4))], axis=2).astype(np.int32)
    h = {f: hashlib.sha256() for f in FIELDS}

    def add(field, *arrays):
        for a in arrays:
            h[field].update(np.ascontiguousarray(a).tobytes())

    def metrics():
        return bytes(eng.metrics_raw())

    def add_features():
        fields = {f for k in feats for f in FEATURE_FIELDS[k]}
        if "fwd_params" in fields:
            add("fwd_params", eng.get_forward_params())
        if "ema" in fields:
            ema, updates = eng.get_ema_state()
            add("ema", ema, np.int64(updates))
            stats, valid = eng.get_ema_bn_state()
            add("ema_bn", stats, np.int64(valid))
        if "norms" in fields:
            add("norms", np.float64(eng.get_grad_norms()))
        return fields

    for s in range(STEPS):
        w = slice(s * B, (s + 1) * B)
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32))
        eng.assemble(win[w], masks[w], 2, 2)
        eng.train_step(B, 1e-2)
        p, z, loss = eng.read_outputs(B)
        add("outputs", p, z, np.float32(loss))
        h["metrics"].update(metrics())
    add("params", eng.get_params())
    m, v, step = eng.get_opt_state()
    add("adam", m, v, np.int64(step))
    add("bn_state", eng.get_bn_state())
    add("grads", eng.get_grads())
    for tname in ("p1", "g1", "bn1"):
        add("debug", eng.debug_read(tname, B, B * T * 64))   # (capacity: no first tensor is wider than 64 channels)
    add_features()
    if feats & {"weight_ema", "bn_reestimate"}:   # (the average holds the copy behind the second step)
        eng.set_option("ema_forward", 1)
    w = slice(STEPS * B, (STEPS + 1) * B)
    eng.assemble(win[w], None, 0, 0)
    eng.forward(B, training=False)
    p, z, _ = eng.read_outputs(B, want_loss=False)
    add("forward", p, z)
    eng.metrics_reset()
    ev = win[(STEPS + 1) * B:]
    if "bn_reestimate" in feats:
        eng.bn_reestimate_windows(ev[:2 * B], B)
        add_features()
    eng.evaluate_windows(ev, (rng.random(ev.shape[0]) < 0.5).astype(np.float32), B)
    h["evaluate"].update(metrics())

    def step(s):
        w = slice(s * B, (s + 1) * B)
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32))
        eng.assemble(win[w], masks[w], 2, 2)
        eng.train_step(B, 1e-2)

    eng.assemble(win[:B], None, 0, 0)
    eng.forward(B, training=True)
    add("sequence", *eng.read_outputs(B, want_loss=False)[:2])
    for s in range(SEQUENCE_STEPS_GRAPHS if options.get("graphs") else SEQUENCE_STEPS):
        step(s % STEPS)
        p, z, loss = eng.read_outputs(B)
        add("sequence", p, z, np.float32(loss))
    add("sequence", eng.get_params())
    if profile:
        eng.set_option("profile", 1)
        eng.profile_read()   # (nothing of the calls above)
        step(0)
        h["profile"].update("\n".join(n for n, _ in eng.profile_read()).encode())
    absent = set(FIELDS[FIELDS.index("profile") + 1:]) - add_features() | (set() if profile else {"profile"})
    eng.close()
    return json.dumps(dict(case=name, **{f: "-" if f in absent else h[f].hexdigest()[:32] for f in FIELDS}))


def compare(path_a, path_b):
    a, b = ({r["case"]: r for r in map(json.loads, open(p))} for p in (path_a, path_b))
    bad = sorted(set(a) ^ set(b))
    for name in a:
        if name in b:
            for f in FIELDS:
                same = a[name][f] == b[name][f]
                print("%-46s %-10s %s %s %s" % (name, f, a[name][f], b[name][f], "equal" if same else "DIFFERENT"))
                if not same:
                    bad.append(name + " " + f)
    print("%d cases, %d hashes: %s" % (len(a), len(a) * len(FIELDS), "all equal" if not bad else "NOT equal: " + ", ".join(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="library to run (default: the package's own)")
    ap.add_argument("--emulator", action="store_true", help="the same cases at the sizes the emulator tests run (a library of tests/hipemu)")
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    from microwakeword_amd import native
    lib = native.NativeLib.get(a.lib)
    for case in cases(a.emulator):
        print(run_case(lib, *case), flush=True)


if __name__ == "__main__":
    main()
