"""Bit identity of the four streaming kernels between two builds of the library: a fixed, seeded set of cases, one JSON line
per case with the sha256 of everything a stream hands back - float probabilities, logits and final float state, calibration
ranges, uint8 outputs and final int8 state.  The kernels sum in a fixed order without atomics, so a change that moves no
arithmetic leaves every hash as it was.

    python tools/stream_identity.py --lib A.so > a.jsonl      # every case (the sizes the GPU tests run)
    python tools/stream_identity.py --lib B.so > b.jsonl
    python tools/stream_identity.py --compare a.jsonl b.jsonl  # two columns, exit status 1 when a hash differs
    python tools/stream_identity.py --lib tests/hipemu/libmww_emu.so --emulator   # the cases the emulator tests run
    python tools/stream_identity.py --variants   # after those, the float cases of tests/mixednet_variant_checks.py and the
                                                 # calibration + int8 cases of tests/quant_mixednet_checks.py
    python tools/stream_identity.py --post       # instead of those: what the five entry points on the probabilities held
                                                 # (csrc/stream_post.hip.h) hand back; the same cases on the GPU and the emulator

The cases: those of tests/stream_sweep.py (the script of each case: several stream-mode calls with resets, zero-output and
one-output calls between them; its non-stream twin), tests/inception_streaming_checks.py ``stream_cases()`` /
``non_stream_cases()`` and tests/quant_graph_checks.py ``cases()``.  Every case runs in stream mode over at least two calls
(the second starts from the rings the first left) and in non-stream mode.  No oracle is consulted: this compares builds.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FIELDS = ("prob", "logit", "state", "ranges", "u8", "state_q8")


class Hashes:
    def __init__(self, fields=FIELDS):
        self.h = {f: hashlib.sha256() for f in fields}

    def add(self, **arrays):
        for f, a in arrays.items():
            self.h[f].update(np.ascontiguousarray(a).tobytes())

    def add_float(self, st):
        p, z = st.read(want_logits=True)
        self.add(prob=p, logit=z, state=st.get_state())

    def add_q8(self, st):
        p, z = st.read(want_logits=True)
        self.add(u8=st.read_q8(), prob=p, logit=z, state_q8=st.get_state_q8())

    def line(self, name):
        return json.dumps(dict(case=name, **{f: h.hexdigest()[:32] for f, h in self.h.items()}))


def run_script(st, model, c, n_cu, add, gen_frames=None):
    """the script of a case (tests/stream_sweep.py) on stream ``st``; ``add(st)`` after every call"""
    import stream_sweep as sw
    import streaming_checks as sc
    gen_frames, s = gen_frames or sw.gen_frames, c.desc["stride"]
    for i, step in enumerate(c.script):
        rng = sw._rng(c.id, 0, i)
        if step[0] == "reset":
            st.reset()
        elif step[0] == "zero":
            st.run_host(gen_frames(rng, s - 1))
        elif step[0] == "tracks":
            st.run(sc.Tracks(model, step[1], step[2], seed=int(rng.integers(1 << 30))).win)
        elif step[0] in ("host", "outputs"):
            n = step[1] if step[0] == "host" else ((2 * n_cu + 2) * sw.TILE + 5 if step[1] == "grid" else step[1]) * s + s - 1
            st.run_host(gen_frames(rng, n, "u16" if i % 2 else "f32"))
        else:
            for _ in range(step[1]):
                st.run_host(gen_frames(rng, s))
                add(st)
        add(st)


def sweep_case(lib, c, n_cu):
    """tests/stream_sweep.py: the case's script on a float and an int8 stream, calibration, the non-stream twin"""
    import stream_sweep as sw
    import streaming_checks as sc
    from microwakeword_amd import native, streaming
    b, H = sw.built(c.id), Hashes()
    model = sc.context_model(lib)
    for kind in ("float", "q8"):
        if kind == "float":
            st = native.Stream(model.engine, b.desc)
            st.set_weights(b.flat)
        else:
            st = streaming.QuantizedStreamingModel(b.qm, b.s, "stream", context=model).native
        add = H.add_float if kind == "float" else H.add_q8
        run_script(st, model, c, n_cu, add)
        if kind == "float":
            st.reset()
            H.add(ranges=st.calibrate_host(b.seq))
            H.add_float(st)
        st.close()
    lens, pads = c.ns
    st = native.Stream(model.engine, dict(b.desc, mode="non_stream"))
    st.set_weights(b.flat)
    st.run(sc.Tracks(model, lens, pads, seed=sw.SEED).win)
    H.add_float(st)
    st.close()
    st = streaming.QuantizedStreamingModel(b.qm, b.s, "non_stream", context=model).native
    st.run(sc.Tracks(model, lens, pads, seed=sw.SEED).win)
    H.add_q8(st)
    st.close()
    return H


def variant_case(lib, c, n_cu):
    """tests/mixednet_variant_checks.py: the case's script on a float stream of mww_stream_create_mixednet (none for a
    spatial-attention case), then its non-stream twin"""
    import mixednet_variant_checks as vc
    import streaming_checks as sc
    b, H = vc.built(c.id), Hashes()
    model = sc.context_model(lib)
    if c.script:
        st = vc.new_stream(lib, b)
        run_script(st, model, c, n_cu, H.add_float)
        st.close()
    st = vc.new_stream(lib, b, "non_stream")
    st.run(sc.Tracks(model, c.ns[0], c.ns[1], seed=vc.SEED).win)
    H.add_float(st)
    st.close()
    return H


def variant_q8_case(lib, cid, n_cu):
    """tests/quant_mixednet_checks.py: calibration on a float stream of mww_stream_create_mixednet_q8, the int8 model of those
    ranges, the case's script on the int8 stream, then its non-stream twin"""
    import mixednet_variant_checks as vc
    import quant_mixednet_checks as qx
    import streaming_checks as sc
    from microwakeword_amd import quantize_mixednet as qmx
    b, H = qx.built(cid), Hashes()
    model = sc.context_model(lib)
    st = qx.new_float_stream(lib, b, True)
    ranges = st.calibrate_host(qx.calibration_frames(cid))
    H.add(ranges=ranges)
    H.add_float(st)
    st.close()
    qm = qmx.quantize_weights(qx.desc_of(b), b.weights, qx._final_ranges(cid, ranges))
    st = qx.new_q8_stream(lib, qm)
    run_script(st, model, b.case, n_cu, H.add_q8, qx.gen_frames)
    st.close()
    st = qx.new_q8_stream(lib, qm, "non_stream")
    st.run(sc.Tracks(model, b.case.ns[0], b.case.ns[1], seed=vc.SEED).win)
    H.add_q8(st)
    st.close()
    return H


def graph_float_case(lib, flags, T, calls, seed, non_stream=None):
    """tests/inception_streaming_checks.py: successive calls on one float graph stream, then non-stream mode"""
    import inception_streaming_checks as ic
    from microwakeword_amd import streaming
    H = Hashes()
    model = ic.make_model(lib, flags, T)[1]
    sm = streaming.StreamingModel(model, 1, "stream")
    for ci, (lengths, pads) in enumerate(calls):
        sm.native.run(ic.Tracks(lengths, pads, seed=seed + ci).upload(model, (2 * ci, 2 * ci + 1)).win)
        H.add_float(sm.native)
    lengths, pads = non_stream or calls[0]
    ns = streaming.StreamingModel(model, 1, "non_stream")
    ns.native.run(ic.Tracks(lengths, pads, seed=seed).upload(model).win)
    H.add_float(ns.native)
    return H


def graph_q8_case(lib, case):
    """tests/quant_graph_checks.py: calibration of the float graph stream, successive calls on the int8 one, non-stream mode"""
    import inception_streaming_checks as ic
    import quant_graph_checks as gc
    import q8_checks as qc
    from microwakeword_amd import native, streaming
    H = Hashes()
    desc, w, qm, _ = case.build()
    model = gc.context_model(lib, case)
    st = native.GraphStream(model.engine, desc, int8=True)
    st.set_weights(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in w]))
    H.add(ranges=st.calibrate_host(qc.calibration_set(gc.CAL_FRAMES, case.cal_seed)))
    H.add_float(st)
    st.close()
    qsm = streaming.QuantizedStreamingModel(qm, 1, "stream", context=model)
    for ci, (lengths, pads) in enumerate(case.calls):
        qsm.native.run(ic.Tracks(lengths, pads, seed=case.seed + ci).upload(model, (2 * ci, 2 * ci + 1)).win)
        H.add_q8(qsm.native)
    ns = streaming.QuantizedStreamingModel(qm, 1, "non_stream", context=model)
    ns.native.run(ic.Tracks(*case.calls[0], seed=case.seed).upload(model).win)
    H.add_q8(ns.native)
    return H


def run(lib, emulator, variants=False):
    import inception_streaming_checks as ic
    import quant_graph_checks as gc
    import stream_sweep as sw
    n_cu = 4 if emulator else 256   # the emulated device has 4 CUs
    small = lambda name: not emulator or name.startswith("emu/")   # noqa: E731
    for c in (sw.emulator_slice() if emulator else sw._cases()):
        print(sweep_case(lib, c, n_cu).line("stream_sweep/" + c.id), flush=True)
    ns = ic.non_stream_cases()
    for name, (flags, T, calls, seed) in ic.stream_cases().items():
        if small(name):
            print(graph_float_case(lib, flags, T, calls, seed, ns[name][2:4] if name in ns else None).line("inception/" + name), flush=True)
    for name, case in gc.cases().items():
        if small(name) or name.startswith("sweep/"):
            print(graph_q8_case(lib, case).line("quant_graph/" + name), flush=True)
    if variants:   # after the existing set, whose output stays as it was
        import mixednet_variant_checks as vc
        for c in vc._cases():
            print(variant_case(lib, c, n_cu).line("mixednet_variant/" + c.id), flush=True)
        import quant_mixednet_checks as qx
        for cid in qx.case_ids():
            print(variant_q8_case(lib, cid, n_cu).line("quant_mixednet/" + cid), flush=True)


def run_post(lib):
    """mww_stream_metrics, _operating_points, _operating_summary, _detections and _mine on the probability set of
    tests/operating_point_checks.py: one line per case of its CASES table (metrics at every window, the grid, the summary),
    one per (window, cooldown, skip, cutoff) of the detection sweep of tests/stream_detect_checks.py (events, track counts,
    best indices, score bits; the clips, events and counts of mining at two max_new, every track ambient)."""
    import itertools
    import engine_checks as ec
    import operating_point_checks as oc
    import stream_detect_checks as dc
    import streaming_checks as sc
    from microwakeword_amd import native
    print(json.dumps(dict(library=lib.version())), flush=True)   # the stamp of the library the hashes are of: not compared
    st = sc.streaming.StreamingModel(sc.make_model(lib, ec.DEF, 52)[1], 1, "stream").native
    inp = oc.inputs()
    n = len(inp.lengths)
    st.set_probs(inp.flat)

    def add(H, field, out):
        for a in out:
            H.h[field].update(np.ascontiguousarray(a).tobytes())

    for name, (cooldown, skip, parity, cutoffs) in oc.CASES.items():
        H = Hashes(("metrics", "points", "summary"))
        kind = np.array([(t + parity) % 2 for t in range(n)], np.int32)
        for w in oc.WINDOWS:
            add(H, "metrics", st.metrics(inp.off, kind, cutoffs, w, skip, cooldown))
        add(H, "points", st.operating_points(inp.off, kind, oc.WINDOWS, cutoffs, skip, cooldown))
        add(H, "summary", st.operating_summary(inp.off, kind, oc.WINDOWS, cutoffs, skip, cooldown, 3, 0.02))
        print(H.line("post/grid/" + name), flush=True)
    win = np.array([(0, t % 3, max(length - t % 3, 0), 0, 40 * int(inp.off[t])) for t, length in enumerate(inp.lengths)], native.WINDOW_DTYPE)
    sweep = list(itertools.product(dc.WINDOWS, dc.COOLDOWNS, dc.SKIPS, dc.CUTOFFS)) + [
        (1, dc.SEG - 1, 0, 0.0), (5, dc.SEG, 25, 0.37), (1, dc.SEG + 1, 0, 0.5), (1, 2500, 0, 0.0)]   # check_against_restatement's
    for window, cooldown, skip, cutoff in sweep:
        H = Hashes(("detections", "mine"))
        kind = np.array([(t + dc.CUTOFFS.index(cutoff)) % 2 for t in range(n)], np.int32)
        add(H, "detections", st.detections(inp.off, kind, cutoff, window, skip, cooldown))
        for max_new in (7, 2000):
            clips, events, total, counts = st.mine(win, inp.off, cutoff, window, cooldown, 2, 3, max_new)
            add(H, "mine", (clips, events, np.int64(total), counts))
        print(H.line("post/events/w%d_cd%d_skip%d_cut%g" % (window, cooldown, skip, cutoff)), flush=True)
    st.close()


def compare(path_a, path_b):
    for p in (path_a, path_b):
        for r in map(json.loads, open(p)):
            if "library" in r:
                print("%s: %s" % (p, r["library"]))
    a, b = ({r["case"]: r for r in map(json.loads, open(p)) if "case" in r} for p in (path_a, path_b))
    bad = sorted(set(a) ^ set(b))
    for name in a:
        if name in b:
            for f in (k for k in a[name] if k != "case"):
                same = a[name][f] == b[name][f]
                print("%-44s %-9s %s %s %s" % (name, f, a[name][f], b[name][f], "equal" if same else "DIFFERENT"))
                if not same:
                    bad.append(name + " " + f)
    print("%d cases, %d hashes: %s" % (len(a), sum(len(r) - 1 for r in a.values()), "all equal" if not bad else "NOT equal: " + ", ".join(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="library to run (default: the package's own)")
    ap.add_argument("--emulator", action="store_true", help="the emulator-sized part of the cases (a library of tests/hipemu)")
    ap.add_argument("--variants", action="store_true", help="also the float cases of tests/mixednet_variant_checks.py (residual, pooled, attention) and the calibration + int8 "
                    "cases of tests/quant_mixednet_checks.py (residual, pooled)")
    ap.add_argument("--post", action="store_true", help="the five entry points on the probabilities a stream holds, instead of the kernels' cases")
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    from microwakeword_amd import native
    if a.post:
        run_post(native.NativeLib.get(a.lib))
    else:
        run(native.NativeLib.get(a.lib), a.emulator, a.variants)


if __name__ == "__main__":
    main()
