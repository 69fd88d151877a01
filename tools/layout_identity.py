"""Identity of the host-side model description between two checkouts: a fixed, seeded list of flag sets, one JSON line per
case with the sha256 of what the layouts, the stream descriptions and the quantizers make of it - ``keras_vars``, ``ops``,
``op_names``, ``engine_args(8)``, ``segments()``, the summary text, ``grad_mask()``, ``pack()`` of seeded weights and every
array of ``unpack(pack(...))`` per layout class; ``stream_description`` / ``mixednet_stream_description`` /
``graph_stream_description`` in both modes; ``tensor_names``, every array of ``packed()``, ``summary()`` and the bytes of
each array of a saved ``.npz`` per quantizer, with seeded ranges.  Where a call raises, the exception's type and message
stand in its place.  All of it is NumPy on the host: no library, no GPU.

    python tools/layout_identity.py > a.jsonl                  # every case, in the checkout the tool is run from
    python tools/layout_identity.py --compare a.jsonl b.jsonl  # one line per case, exit status 1 when a field differs

The cases: the default, notebook, graph and synthetic MixedNet flag sets, the default Inception (both ``fuse_heads``), the
flag sets of the streaming variant sweep, 40 random MixedNet and 40 random Inception flag sets, and the refusals the tests
pin (no first convolution, kernel size 1, descending kernel sizes, too few frames, lists of different lengths, attention
over fewer than four frames, attention in stream mode).  No oracle is consulted: this compares checkouts.
"""
import argparse
import collections
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SEEDS = range(40)


def cases():
    """(name, family, flags, frames)"""
    import engine_checks as ec
    import mixednet_variant_checks as mv
    from microwakeword_amd import synthetic
    out = [("mixednet/default", "mixednet", ec.DEF, 194), ("mixednet/notebook", "mixednet", ec.NOTEBOOK, 204),
           ("mixednet/graph", "mixednet", ec.GRAPH_MIXEDNET, 100), ("mixednet/synthetic", "mixednet", synthetic.DEFAULT_MIXEDNET_FLAGS, 194),
           ("inception/default", "inception", ec.INC, 194)]
    out += [("variant/" + c.id, "mixednet", mv.flags_of(c.desc), c.desc["frames"]) for c in mv.cases()]
    out += [("mixednet/random%d" % s, "mixednet", ec.random_mixednet_flags(s), 70) for s in SEEDS]
    out += [("inception/random%d" % s, "inception", ec.random_inception_flags(s), 150) for s in SEEDS]
    att = dict(ec.DEF, spatial_attention=1)
    out += [("refusal/no-first-conv", "mixednet", dict(ec.DEF, first_conv_filters=0), 194),
            ("refusal/kernel-size-1", "mixednet", dict(ec.DEF, mixconv_kernel_sizes="[5],[1],[13],[21]"), 194),
            ("refusal/kernel-size-1-first", "mixednet", dict(ec.DEF, mixconv_kernel_sizes="[1],[9],[13],[21]"), 30),
            ("refusal/descending-kernels", "mixednet", dict(ec.DEF, mixconv_kernel_sizes="[5],[11,7],[13],[21]"), 194),
            ("refusal/descending-kernels-short", "mixednet", dict(ec.DEF, mixconv_kernel_sizes="[5],[9],[13],[21,3]"), 30),
            ("refusal/too-short", "mixednet", ec.DEF, 40), ("refusal/shorter-than-first-conv", "mixednet", ec.NOTEBOOK, 4),
            ("refusal/too-short-graph", "mixednet", ec.GRAPH_MIXEDNET_RESIDUAL, 12),
            ("refusal/list-lengths", "mixednet", dict(ec.DEF, residual_connection="0,0,0,0,0"), 194),
            ("refusal/list-lengths-repeat", "mixednet", dict(ec.DEF, repeat_in_block="1,1,1", spatial_attention=1), 20),
            ("refusal/attention-3-frames", "mixednet", att, 3 + 44 + 2), ("refusal/attention-1-frame", "mixednet", att, 1 + 44 + 2),
            ("refusal/attention-stream", "mixednet", att, 194), ("refusal/attention-pooled-residual", "mixednet", ec.GRAPH_MIXEDNET_FULL, 194),
            ("refusal/inception-too-short", "inception", ec.INC, 20),
            ("refusal/inception-groups", "inception", dict(ec.INC, cnn1_subspectral_groups="5"), 194)]
    return out


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def text_digest(obj):
    return hashlib.sha256(repr(obj).encode()).hexdigest()[:32]


def guarded(record, key, fn):
    """fn() -> {field: value}, stored under key.field; an exception is the value of key itself"""
    try:
        for k, v in fn().items():
            record[key + "." + k] = v
        return True
    except Exception as e:   # noqa: BLE001 - the refusal is what is recorded
        record[key] = "%s: %s" % (type(e).__name__, e)
        return False


def seeded_weights(lay, rng):
    out = []
    for name, shape, _ in lay.keras_vars:
        w = rng.normal(0.0, 0.5, shape).astype(np.float32)
        out.append(np.abs(w) + np.float32(0.25) if name.endswith(("variance", "gamma")) else w)
    return out


def layout_fields(make, rng, keep):
    def run():
        lay = make()
        keep.append(lay)
        ws = seeded_weights(lay, rng)
        p, s = lay.pack(ws)
        back = lay.unpack(p, s)
        return dict(keras_vars=text_digest(lay.keras_vars), ops=text_digest(getattr(lay, "ops", None)),
                    op_names=text_digest(getattr(lay, "op_names", None)), engine_args=text_digest(lay.engine_args(8)),
                    segments=text_digest(lay.segments()), summary=text_digest("\n".join(lay.summary_lines())),
                    counts=text_digest((lay.keras_param_counts(), lay.n_params, lay.n_state, lay.t_last, lay.c_last)),
                    grad_mask=digest(lay.grad_mask()), pack=digest(p, s), unpack=digest(*back),
                    round_trip=all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(ws, back)) and len(ws) == len(back))
    return run


def quantizer_fields(module, desc, weights, rng):
    def run():
        names = module.tensor_names(desc)
        lo = -rng.random(len(names)) * 4.0
        ranges = np.stack([lo, lo + 0.5 + rng.random(len(names)) * 8.0], 1)
        q = module.quantize_weights(desc, weights, ranges)
        buf = io.BytesIO()
        q.save(buf)
        buf.seek(0)
        with np.load(buf, allow_pickle=False) as z:
            saved = digest(*[np.frombuffer(k.encode(), np.uint8) for k in z.files], *[z[k] for k in z.files])
        return dict(tensor_names=text_digest(names), desc=text_digest(q.desc), packed=digest(*q.packed()), summary=text_digest(q.summary()),
                    npz=saved)
    return run


def run_case(name, family, flags, frames):
    from microwakeword_amd import layout, quantize, quantize_graph, quantize_mixednet, streaming
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    rec = dict(case=name)
    if family == "inception":
        for fuse in (True, False):
            keep = []
            guarded(rec, "InceptionLayout[fuse_heads=%d]" % fuse, layout_fields(lambda: layout.InceptionLayout(flags, frames, fuse_heads=fuse), rng, keep))
        for mode in ("stream", "non_stream"):
            guarded(rec, "graph_stream_description[%s]" % mode, lambda: dict(desc=text_digest(streaming.graph_stream_description(flags, frames, 1, mode))))
        if keep:
            guarded(rec, "quantize_graph", quantizer_fields(quantize_graph, streaming.graph_stream_description(flags, frames, 1, "stream"),
                                                            seeded_weights(keep[0], rng), rng))
        guarded(rec, "inception_slices_dropped", lambda: dict(n=layout.inception_slices_dropped(flags)))
        return rec
    lays = {}
    for cls in (layout.MixedNetLayout, layout.GraphMixedNetLayout):
        keep = []
        if guarded(rec, cls.__name__, layout_fields(lambda: cls(flags, frames), rng, keep)):
            lays[cls.__name__] = keep[0]
    stride = int(flags["stride"])
    any_lay = lays.get("GraphMixedNetLayout") or lays.get("MixedNetLayout")
    descs = {}
    for mode in ("stream", "non_stream"):
        for t_final in sorted({1, any_lay.t_last if any_lay else 1}):
            key = "stream_description[%s,t_final=%d]" % (mode, t_final)
            guarded(rec, key, lambda: dict(desc=text_digest(streaming.stream_description(flags, t_final, frames, stride, mode))))
        key = "mixednet_stream_description[%s]" % mode
        guarded(rec, key, lambda: dict(desc=text_digest(descs.setdefault(key, streaming.mixednet_stream_description(flags, frames, stride, mode)))))
        guarded(rec, "stream_description[%s,stride+1]" % mode, lambda: dict(desc=text_digest(streaming.stream_description(flags, 1, frames, stride + 1, mode))))
        guarded(rec, "mixednet_stream_description[%s,stride+1]" % mode,
                lambda: dict(desc=text_digest(streaming.mixednet_stream_description(flags, frames, stride + 1, mode))))
    guarded(rec, "mixednet_variant_flags", lambda: dict(names=text_digest(streaming.mixednet_variant_flags(flags))))
    guarded(rec, "spectrogram_slices_dropped", lambda: dict(n=layout.spectrogram_slices_dropped(flags)))
    for mode in ("stream", "non_stream"):
        guarded(rec, "check_evaluation_topology[%s]" % mode, lambda: dict(
            ok=streaming.check_evaluation_topology(flags, frames, stride, [mode], int8=True) is None))
        guarded(rec, "check_evaluation_topology[%s,int8_variants]" % mode, lambda: dict(
            ok=streaming.check_evaluation_topology(flags, frames, stride, [mode], int8=True, int8_variants=True) is None))
    general = descs.get("mixednet_stream_description[stream]") or descs.get("mixednet_stream_description[non_stream]")
    if any_lay is not None and general is not None:   # the quantizers: the general one on every description, both on a plain one
        ws = seeded_weights(any_lay, rng)
        guarded(rec, "quantize_mixednet[general description]", quantizer_fields(quantize_mixednet, general, ws, rng))
        if not (any(general["residual"]) or general["attention"] or general["pool"]):
            plain = streaming.stream_description(flags, general["t_final"], frames, stride, "stream")
            guarded(rec, "quantize_mixednet[plain description]", quantizer_fields(quantize_mixednet, plain, ws, rng))
            guarded(rec, "quantize[plain description]", quantizer_fields(quantize, plain, ws, rng))
            guarded(rec, "quantize[general description]", quantizer_fields(quantize, general, ws, rng))
    return rec


def compare(path_a, path_b):
    """one line per case: the number of fields, how many of them are refusals, and the sha256 over all of a's and of b's fields;
    under a case that differs, every field that does"""
    a, b = ({r["case"]: r for r in map(json.loads, open(p))} for p in (path_a, path_b))
    bad = sorted(set(a) ^ set(b))
    n = 0
    for name in a:
        if name not in b:
            continue
        fields = sorted((set(a[name]) | set(b[name])) - {"case"})
        n += len(fields)
        refusals = sum(isinstance(a[name].get(f), str) and ": " in a[name][f] for f in fields)
        ha, hb = (text_digest([(f, r[name].get(f, "<absent>")) for f in fields]) for r in (a, b))
        print("%-58s %3d fields %3d refusals  %s %s %s" % (name, len(fields), refusals, ha, hb, "equal" if ha == hb else "DIFFERENT"))
        for f in fields:
            va, vb = a[name].get(f, "<absent>"), b[name].get(f, "<absent>")
            if va != vb:
                print("    %s: %s -> %s" % (f, va, vb))
                bad.append(name + " " + f)
    print("%d cases, %d fields: %s" % (len(a), n, "all equal" if not bad else "NOT equal: " + ", ".join(bad)))
    print("the refusals among them (times in a, times in b; the call, the start of the message):")
    tally = [collections.Counter((f.split("[")[0], v[:96]) for r in side.values() for f, v in r.items()
                                 if f != "case" and isinstance(v, str) and ": " in v) for side in (a, b)]
    for key in sorted(set(tally[0]) | set(tally[1])):
        print("  %4d %4d  %-28s %s" % (tally[0][key], tally[1][key], key[0], key[1]))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    for case in cases():
        print(json.dumps(run_case(*case)), flush=True)


if __name__ == "__main__":
    main()
