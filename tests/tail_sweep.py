"""A covering sweep of the kernels every train step of either engine ends in - head_kernel, dense_grad_kernel / dense_grad_body,
metrics_body<256> / <1024> (csrc/kernels_head.hip.h), head_tail_kernel and grad_final_kernel (kernels_tail.hip.h), adam_kernel and
the launch code around them in mww_lib.hip - shared by the GPU sweep (tests/test_tail_sweep_gpu.py) and its CPU-side checks
(tests/test_tail_sweep_emulated.py).  The manner of tests/graph_table_sweep.py:

- ``head_table()`` reads the X(C, J) list out of launch_head in mww_lib.hip itself (a new instantiation becomes required without
  anyone editing this file; a shape the parser does not understand is a ValueError);
- ``inventory()`` is every instantiation of the family: head_kernel<C, J, SB>, the eight dense_role_chunks<SB, RES, KEEP> of
  grad_final_kernel, the eight row loops of dense_grad_body (named dense_grad_body<SB, RES, KEEP>), the three metric workgroup
  forms, the two Adam forms;
- ``required()`` adds the axis items of the module constants below; ``plan()`` is a deterministic list of cases that covers
  them; ``uncovered()`` must equal ``UNREACHABLE`` exactly - a flag set that reaches a listed instantiation turns the coverage
  test red;
- ``run_case()`` runs a case against tests/tail_oracle.py, the float64 restatement fed with the engine's own head inputs, at
  derived bounds, and returns the worst error of every quantity as a fraction of its bound (a NaN or inf of the engine counts
  as an error without bound, and every value read back is asserted finite).

What the coverage is and is not.  The items of a case are DECLARED by the plan from the host code as read (block engine with
"bn_inline" and "tail_roles": the dense role of grad_final; otherwise head_tail; graph engine: enqueue_side_work), they are not
observed: no read-back tells which dense_role_chunks<SB, RES, KEEP> a launch ran, so a flag set that newly routed a residual or
dropout source into grad_final's dense role would stay unnoticed until the plan is relabelled - UNREACHABLE records today's
reading of tail_src.  What a case does check of its route are the launch NAMES of one MORE step under "profile" after the compared
ones (captured graphs are not replayed under "profile").  In the block engine that step launches what the compared steps
launched.  In the graph engine "profile" itself moves the side work onto the main stream and, with the metric update, into the
one-launch form, so the profiled step names dense_grad_kernel only without the metric update: there the names show that the form
exists and is wired, not what the compared steps launched.

Axis items (the terms of required() next to the instantiation names):
  ("edge", head instantiation, "upper" | "lower", grid)   T_final = NRG * J, and one frame past the previous J's upper edge
                                        (T_final = 1 for J = 2), B = 3 under "grid_head" 1 (three windows through the prefetch
                                        chain), 2 (an uneven deal) and 0 = the default (one window each)
  ("partial-row-group", 48)             a T_final that is no multiple of the 21 frame groups of 48 channels
  ("mode", C, name)                     acc / gstat-tail0 / gstat-inline0 / clipped / eval-metrics / forward / zero-weights per C,
                                        gstat-gridmax (grid_head at its maximum, B above it) once
  ("batch", T_final, B, route)          route "A" (grad_final's dense role), "B" (head_tail's chunk rows summed as partial rows;
                                        asserts A == B bit for bit), "metrics1024" (forward with update_metrics)
  ("graph", form, B)                    the graph engine's routes: plain / res / res-rdrop / keep / res+keep / one-launch
  ("segments>56",)                      a gradient assembly of more than kMaxFinalSegments segments (two grad_final launches)
  ("partials", B, grid_bwd)             grad_final kind 0 through engine_checks.check_train_steps, unchanged
  ("metric-edge", bias, label, form), ("cumulative",), ("adam", "3-steps" | "fused==apply"), ("mixconv-zeros",),
  ("replay", "A" | "B" | "graph")

The input condition of every train case (tail_oracle.head_input_condition / dense_input_condition) is computed from the float64
oracle alone by ``input_condition(case)``; the dense kernel of a case is drawn with magnitudes in [0.5, 1] x 2 / sqrt(n) so that no
frame row hides below the bound of z.  The metric-edge cases are exempt: their dense kernel is exact zeros by construction."""
import functools
import os
import re

import numpy as np

import tail_oracle as to
from oracle import model_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MWW_LIB = os.path.join(ROOT, "microwakeword_amd", "csrc", "mww_lib.hip")

HEAD_WIDTHS_BF16 = (48, 64)   # last-block widths of MWW_BLOCK_SHAPES_BF16 (block_launch.hip.h); the emulated test holds the library to it
GRID_HEAD_MAX_PER_CU = 4      # option table of mww_lib.hip: "grid_head" <= 4 x CUs
MI355X_CUS = 256
BATCHES = (1, 2, 31, 32, 33, 65, 255, 256, 257, 1023, 1024, 1025, 1057)
GRAPH_BATCHES = (5, 33, 288)
MODES = ("acc", "gstat-tail0", "gstat-inline0", "clipped", "eval-metrics", "forward", "zero-weights")
EDGE_BIASES = (0.0, 40.0, -40.0, -110.0)
K_RING = 8                    # kRing (engine.hip.h): mailbox slots; a captured train step is keyed on its slot
REPLAY_STEPS = 2 * K_RING + 2


# ------------------------------------------------------------------------------------------ the head table
def _parse_head_table(text):
    m = re.search(r"\bint launch_head\(.*?\n\}", text, re.S)
    if not m:
        raise ValueError("mww_lib.hip: launch_head not found")
    body = m.group(0)
    d = re.search(r"#define X\(C, J\)(?:[^\n]*\\\n)*[^\n]*\n(.*?)#undef X", body, re.S)
    if not d:
        raise ValueError("launch_head: no '#define X(C, J)' ... '#undef X' block")
    rows = "\n".join(l for l in d.group(1).split("\n") if not l.strip().startswith(("static_assert", "//")))
    entries = re.findall(r"X\(([^()]*)\)", rows)
    if re.sub(r"X\([^()]*\)", "", rows).strip():
        raise ValueError("launch_head: cannot parse %r" % re.sub(r"X\([^()]*\)", "", rows).strip())
    out = []
    for e in entries:
        try:
            row = tuple(int(v) for v in e.split(","))
        except ValueError:
            raise ValueError("launch_head: entry X(%s) is not a list of integers" % e) from None
        if len(row) != 2:
            raise ValueError("launch_head: entry X(%s) has %d fields, not 2" % (e, len(row)))
        out.append(row)
    if not out:
        raise ValueError("launch_head: empty instantiation list")
    # launch_head takes the FIRST entry with ch == C && jmax <= J: the rows of a width must ascend for the lower edges below
    for c in {c for c, _ in out}:
        js = [j for cc, j in out if cc == c]
        if js != sorted(set(js)):
            raise ValueError("launch_head: the J of %d channels do not ascend" % c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _head_table(path):
    with open(path) as fh:
        return _parse_head_table(fh.read())


def head_table(path=MWW_LIB):
    """((C, J), ...) of launch_head, in its order."""
    return _head_table(path)


def head_inst(C, J, sb):
    return "head_kernel<%d, %d, %s>" % (C, J, "true" if sb else "false")


def head_j(C, t_final, table=None):
    """The J launch_head picks for t_final frames at C channels (None: no instantiation)."""
    need = -(-t_final // to.head_groups(C))
    for c, j in table or head_table():
        if c == C and need <= j:
            return j
    return None


def head_edges(C, J, table=None):
    """(lower, upper) T_final of head_kernel<C, J>."""
    js = [j for c, j in table or head_table() if c == C]
    prev = max([j for j in js if j < J], default=0)
    return (prev * to.head_groups(C) + 1, J * to.head_groups(C))


def _tf(v):
    return "true" if v else "false"


def dense_role(sb, res, keep):
    return "dense_role_chunks<%s, %s, %s>" % (_tf(sb), _tf(res), _tf(keep))


def dense_body(sb, res, keep):
    return "dense_grad_body<%s, %s, %s>" % (_tf(sb), _tf(res), _tf(keep))


_PLAIN = ("metrics_body<256>@grad_final", "metrics_body<256>@head_tail", "metrics_body<1024>", "grad_final_kernel+adam", "adam_kernel",
          "head_tail_kernel", "dense_grad_kernel", "grad_final_kernel:partials")


def inventory(table=None):
    inv = set(_PLAIN)
    for c, j in table or head_table():
        inv |= {head_inst(c, j, False), head_inst(c, j, True)}
    for sb in (False, True):
        for res in (False, True):
            for keep in (False, True):
                inv |= {dense_role(sb, res, keep), dense_body(sb, res, keep)}
    return frozenset(inv)


def _unreachable(table):
    un = {}
    for c, j in table:
        if c not in HEAD_WIDTHS_BF16:
            un[head_inst(c, j, True)] = ("mww_block_kernels_cover refuses \"storage_bf16\" for a model whose last block is %d wide "
                                         "(MWW_BLOCK_SHAPES_BF16 holds 48 x 48 and 64 x 64 blocks only)" % c)
    for sb in (False, True):
        for res in (False, True):
            for keep in (False, True):
                if res or keep:
                    un[dense_role(sb, res, keep)] = ("only the block engine sets tail_in_reduce, and its tail_src has rp = keep = nullptr: the residual and "
                                                     "dropout forms run in dense_grad_body only, from the graph engine (suspected dead code)")
                    if sb:
                        un[dense_body(sb, res, keep)] = "the graph engine has no bf16 mode (p_bf16 = 0) and the block engine no residual branch or dropout"
    un[("graph-flags", "res+keep")] = ("no flag set: the MixedNet layouts create their engine with dropout 0, Inception has no residual branch "
                                       "(the sweep runs the form through Engine(conv_ops=..., dropout=...) directly)")
    return un


UNREACHABLE = _unreachable(head_table())


def required(table=None):
    t = table or head_table()
    un = _unreachable(t)
    req = set(inventory(t)) | set(un)
    for c, j in t:
        for sb in (False, True):
            if head_inst(c, j, sb) in un:
                continue
            req |= {("edge", head_inst(c, j, sb), e, g) for e in ("upper", "lower") for g in (1, 2, 0)}
    widths = sorted({c for c, _ in t})
    req |= {("partial-row-group", 48)}
    req |= {("mode", c, m) for c in widths for m in MODES} | {("mode", widths[0], "gstat-gridmax")}
    req |= {("batch", tf, b, r) for tf in (8, 9) for b in BATCHES for r in ("A", "B", "metrics1024")}
    req |= {("graph", f, b) for f in ("plain", "res", "res-rdrop", "keep", "res+keep", "one-launch") for b in GRAPH_BATCHES}
    req |= {("segments>56",)}
    req |= {("partials", 9, 9), ("partials", 65, 65), ("partials", 257, 0)}
    req |= {("metric-edge", b, lab, f) for b in EDGE_BIASES for lab in (0, 1) for f in ("logits", "clipped")}
    req |= {("cumulative",), ("adam", "3-steps"), ("adam", "fused==apply"), ("mixconv-zeros",)}
    req |= {("replay", r) for r in ("A", "B", "graph")}
    return frozenset(req)


# ------------------------------------------------------------------------------------------ cases
def block_flags(C, sb=False, kernels=None):
    """The smallest block-engine MixedNet ending in C channels: conv1 3 x 32 and two blocks (3-tap; 5-tap under bf16 storage,
    whose table starts there)."""
    k = 5 if sb else 3
    ks = kernels or "[%d],[%d]" % (k, k)
    f = dict(mo.MIXEDNET_DEFAULTS, pointwise_filters="%d,%d" % (C, C), repeat_in_block="1,1", residual_connection="0,0",
             mixconv_kernel_sizes=ks, first_conv_filters=32, first_conv_kernel_size=3, stride=1)
    if sb:
        f["st_bf16"] = True
    return f


def block_frames(t_final, sb=False, taps=None):
    return t_final + 2 + (taps if taps is not None else 2 * ((5 if sb else 3) - 1))


def graph_flags(form, blocks=2):
    """Small graph-engine MixedNets with widths of MWW_G_WIDTHS: 16 -> 16 -> 24 channels, the last block with a residual branch
    ("res": a 1-tap block, residual_drop 0; "res-rdrop": 3 taps, residual_drop 2)."""
    res = form in ("res", "res-rdrop", "res+keep")
    widths = [16] * (blocks - 1) + [24]
    ks = ["[3]"] * (blocks - 1) + ["[1]" if form == "res" else "[3]"]
    return dict(mo.MIXEDNET_DEFAULTS, pointwise_filters=",".join(map(str, widths)), repeat_in_block=",".join(["1"] * blocks),
                residual_connection=",".join(["0"] * (blocks - 1) + ["1" if res else "0"]), mixconv_kernel_sizes=",".join(ks),
                first_conv_filters=16, first_conv_kernel_size=3, stride=1)


def _case(cid, kind, engine, flags, T, B, **kw):
    c = dict(id=cid, kind=kind, engine=engine, flags=flags, T=int(T), B=int(B), grid_head=0, options={}, mode="train", weights="mixed",
             steps=1, lrs=(1e-3,), graphs=0, seed=42, items=(), dropout=0.0, expect=(), forbid=())
    c.update(kw)
    return c


def _train_expect(options):
    """profile names a block-engine train step must / must not record"""
    late = options.get("bn_inline", 1) and options.get("tail_roles", 1)
    return (("head", "grad_final+adam"), ("head_tail",)) if late else (("head", "head_tail", "grad_final+adam"), ())


def _route_items(sb, options):
    late = options.get("bn_inline", 1) and options.get("tail_roles", 1)
    if late:
        return {dense_role(sb, False, False), "metrics_body<256>@grad_final", "grad_final_kernel+adam"}
    return {dense_body(sb, False, False), "metrics_body<256>@head_tail", "head_tail_kernel", "grad_final_kernel+adam", "grad_final_kernel:partials"}


@functools.lru_cache(maxsize=None)
def _plan(path):
    table = head_table(path)
    un = _unreachable(table)
    cases = []
    widths = sorted({c for c, _ in table})
    # 1. head edges x grids
    for C, J in table:
        for sb in (False, True):
            inst = head_inst(C, J, sb)
            if inst in un:
                continue
            lo, hi = head_edges(C, J, table)
            for edge, tf in (("upper", hi), ("lower", lo)):
                for g in (1, 2, 0):
                    ex, fb = _train_expect({})
                    cases.append(_case("head%dx%d%s-%s-grid%s" % (C, J, "st" if sb else "", edge, g or "auto"), "train", "block", block_flags(C, sb),
                                       block_frames(tf, sb), 3, grid_head=g, C=C, sb=sb, t_final=tf, expect=ex, forbid=fb,
                                       items=(inst, ("edge", inst, edge, g)) + tuple(_route_items(sb, {}))))
    # 2. a partial last row group at 48 channels (21 frame groups), and the head modes at one shape per width
    cases.append(_case("head48x%d-partial-row-group" % head_j(48, 50, table), "train", "block", block_flags(48), block_frames(50), 3, grid_head=2, C=48, sb=False,
                       t_final=50, expect=_train_expect({})[0], forbid=_train_expect({})[1],
                       items=(("partial-row-group", 48), head_inst(48, head_j(48, 50, table), False))))
    for C in widths:
        tf = 2 * to.head_groups(C) + 5   # three frame rows per thread (J = 4 of the list as it stands) with a partial last row group
        base = dict(C=C, sb=False, t_final=tf)
        for name, kw in (("acc", dict(options={"bn_inline": 1, "tail_roles": 1}, B=5, grid_head=2)),
                         ("gstat-tail0", dict(options={"tail_roles": 0}, B=5, grid_head=2)),
                         ("gstat-inline0", dict(options={"bn_inline": 0}, B=5, grid_head=2)),
                         ("clipped", dict(options={"bce_from_logits": 0}, B=5, grid_head=2)),
                         ("eval-metrics", dict(mode="eval-metrics", B=5, grid_head=2)),
                         ("forward", dict(mode="forward", B=5, grid_head=2)),
                         ("zero-weights", dict(weights="zeros", B=6, grid_head=4))):
            kw = dict(base, **kw)
            opts = kw.get("options", {})
            mode = kw.get("mode", "train")
            ex, fb = _train_expect(opts) if mode == "train" else ((("head", "metrics"), ()) if mode == "eval-metrics" else (("head",), ("metrics",)))
            items = [("mode", C, name), head_inst(C, head_j(C, tf, table), False)]
            items += list(_route_items(False, opts)) if mode == "train" else (["metrics_body<1024>"] if mode == "eval-metrics" else [])
            B = kw.pop("B")
            cases.append(_case("head%d-%s" % (C, name), "train" if mode == "train" else mode, "block", block_flags(C), block_frames(tf), B, expect=ex, forbid=fb,
                               items=tuple(items), **kw))
    C = widths[0]
    gmax = GRID_HEAD_MAX_PER_CU * MI355X_CUS
    cases.append(_case("head%d-gstat-gridmax" % C, "train", "block", block_flags(C), block_frames(8), gmax + gmax // 2, grid_head=-1, C=C, sb=False, t_final=8,
                       options={"tail_roles": 0}, expect=_train_expect({"tail_roles": 0})[0], items=(("mode", C, "gstat-gridmax"),)))
    # 3. the batch axis on the smallest model: T_final x C = 256 (the bias gradient alone in the second dense_grad workgroup and in
    # the ninth grad_final column group) and 9 frames
    for tf in (8, 9):
        for B in BATCHES:
            for route, opts in (("A", {}), ("B", {"tail_roles": 0})):
                ex, fb = _train_expect(opts)
                cases.append(_case("dense-T%d-B%d-route%s" % (tf, B, route), "train", "block", block_flags(32), block_frames(tf), B, C=32, sb=False, t_final=tf,
                                   options=opts, route=route, expect=ex, forbid=fb, items=(("batch", tf, B, route),) + tuple(_route_items(False, opts))))
            cases.append(_case("dense-T%d-B%d-metrics1024" % (tf, B), "eval-metrics", "block", block_flags(32), block_frames(tf), B, C=32, sb=False, t_final=tf,
                               mode="eval-metrics", expect=("head", "metrics"), items=(("batch", tf, B, "metrics1024"), "metrics_body<1024>")))
    # (bf16 storage through head_tail: the SB form of dense_grad_body, and of the dense role)
    for route, opts in (("A", {}), ("B", {"tail_roles": 0})):
        ex, fb = _train_expect(opts)
        cases.append(_case("dense-st48-B33-route%s" % route, "train", "block", block_flags(48, True), block_frames(9, True), 33, C=48, sb=True, t_final=9,
                           options=opts, expect=ex, forbid=fb, items=tuple(_route_items(True, opts))))
    # 4. the graph engine's routes
    for form in ("plain", "res", "res-rdrop", "keep", "res+keep", "one-launch"):
        res, keep = form.startswith("res"), form.endswith("keep")
        for B in GRAPH_BATCHES:
            one = form == "one-launch"
            items = [("graph", form, B), dense_body(False, res, keep), "grad_final_kernel+adam", "grad_final_kernel:partials"]
            items += ["head_tail_kernel", "metrics_body<256>@head_tail"] if one else ["dense_grad_kernel", "metrics_body<1024>"]
            cases.append(_case("graph-%s-B%d" % (form, B), "graph", "graph", graph_flags(form), 24, B, options={"side_stream": 0} if one else {},
                               dropout=0.25 if keep else 0.0, form=form, items=tuple(items)))
    cases.append(_case("graph-segments", "graph", "graph", graph_flags("plain", blocks=14), 40, 5, form="plain", items=(("segments>56",),), two_finals=True))
    # (... and the numbers of both launches against the whole-step float64 oracle; on the emulated kernels this model takes half a
    # minute, so the emulated slice keeps to the case above: the route, the dense gradient and Adam)
    cases.append(_case("graph-segments-whole-step", "graph-whole-step", "graph", graph_flags("plain", blocks=14), 40, 5, items=("grad_final_kernel:partials",)))
    # 5. grad_final kind 0: partial-row sums through check_train_steps, unchanged
    for B, g in ((9, 9), (65, 65), (257, 0)):
        cases.append(_case("partials-B%d-grid%s" % (B, g or "auto"), "partials", "block", dict(block_flags(32), residual_connection="0,0"), block_frames(8), B,
                           grid=g, items=(("partials", B, g), "grad_final_kernel:partials")))
    # 6. metric buckets at p = 0.5, 1, ~4e-18 and 0, both labels (within one batch), both loss forms
    for bias in EDGE_BIASES:
        for form in ("logits", "clipped"):
            cases.append(_case("metrics-p%s-%s" % ({0.0: "0.5", 40.0: "1", -40.0: "tiny", -110.0: "0"}[bias], form), "metric-edge", "block", block_flags(32),
                               block_frames(8), 8, bias=bias, options={} if form == "logits" else {"bce_from_logits": 0},
                               items=tuple(("metric-edge", bias, lab, form) for lab in (0, 1))))
    # 7. cumulative state across the three metric forms, Adam, structural zeros, graph replay
    cases.append(_case("metrics-cumulative", "cumulative", "block", block_flags(32), block_frames(8), 1025, sizes=(257, 1025), items=(("cumulative",),)))
    # (the same sequence with 129 and 257 in the places of 257 and 1025: what the emulated kernels run)
    cases.append(_case("metrics-cumulative-B257", "cumulative", "block", block_flags(32), block_frames(8), 257, sizes=(129, 257), items=()))
    cases.append(_case("adam-3-steps", "train", "block", block_flags(32), block_frames(8), 8, C=32, sb=False, t_final=8, steps=3, lrs=(1e-3, 3e-3, 5e-4),
                       expect=_train_expect({})[0], items=(("adam", "3-steps"),)))
    cases.append(_case("adam-fused-equals-apply", "adam-apply", "block", block_flags(32), block_frames(8), 8, steps=3, lrs=(1e-3, 3e-3, 5e-4),
                       items=(("adam", "fused==apply"), "adam_kernel")))
    cases.append(_case("mixconv-structural-zeros", "mixconv", "block", block_flags(32, kernels="[3,5],[3]"), block_frames(8, taps=6), 8, steps=3,
                       lrs=(1e-3, 3e-3, 5e-4), items=(("mixconv-zeros",),)))
    # A captured step is keyed on its mailbox slot (the Adam node reads hyper[] there; mail_commit moves on after every step, the
    # ring has kRing = 8 slots) and on the accumulator parities of the statistics hand-over (period 2): steps 1 .. 8 each capture
    # a graph of their own, step 9 is the first to launch a cached one again.  REPLAY_STEPS = 2 * kRing + 2 launches the execs of
    # steps 1 and 2 - both parities - three times each (steps 1 / 9 / 17 and 2 / 10 / 18: two replays), every time with a new
    # batch, new labels and a new learning rate in the slot.
    lrs = tuple((1e-3, 3e-3, 5e-4)[k % 3] for k in range(REPLAY_STEPS))
    for route, opts in (("A", {}), ("B", {"tail_roles": 0})):
        cases.append(_case("replay-route%s" % route, "train", "block", block_flags(32), block_frames(9), 5, C=32, sb=False, t_final=9, options=opts, graphs=1,
                           steps=REPLAY_STEPS, lrs=lrs, items=(("replay", route),)))
    cases.append(_case("replay-graph", "graph", "graph", graph_flags("plain"), 24, 5, form="plain", graphs=1, steps=REPLAY_STEPS, lrs=lrs,
                       items=(("replay", "graph"),)))
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return tuple(cases)


def plan(path=MWW_LIB):
    return [dict(c, flags=dict(c["flags"]), options=dict(c["options"])) for c in _plan(path)]


def case_items(case):
    return set(case["items"])


def uncovered(path=MWW_LIB):
    """Items of required() that plan() does not cover: UNREACHABLE when the plan is complete."""
    cov = set()
    for c in plan(path):
        cov |= case_items(c)
    return sorted(set(required(head_table(path))) - cov, key=str)


def emulator_slice(path=MWW_LIB):
    """The slice of the plan the emulated kernels run: every route, every C with its smallest and largest J (upper edge under
    grid 1 - three windows through the prefetch chain - and lower edge under grid 2), every head mode at one width and the
    gstat / clipped modes at all, the metric-edge and cumulative cases, B in {33, 65} on the batch axis, every graph form at
    B = 33, Adam, the structural zeros and one replay."""
    table = head_table(path)
    js = {c: [j for cc, j in table if cc == c] for c in {c for c, _ in table}}
    keep = set()
    for c, jj in js.items():
        keep |= {"head%dx%d-upper-grid1" % (c, jj[0]), "head%dx%d-lower-grid2" % (c, jj[0]), "head%dx%d-upper-grid1" % (c, jj[-1]), "head%dx%d-lower-grid2" % (c, jj[-1])}
        keep |= {"head%d-%s" % (c, m) for m in ("gstat-tail0", "clipped")}
    keep |= {"head48x%dst-upper-gridauto" % js[48][0], "head64x%dst-lower-grid1" % js[64][-1], "head48x%d-partial-row-group" % head_j(48, 50, table)}
    keep |= {"head32-%s" % m for m in MODES}
    keep |= {"dense-T%d-B%d-%s" % (tf, b, r) for tf in (8, 9) for b in (33, 65) for r in ("routeA", "routeB", "metrics1024")}
    keep |= {"dense-st48-B33-routeA", "dense-st48-B33-routeB", "graph-segments"}   # (the partials cases' grids exceed the emulated device's 4 CUs)
    keep |= {"graph-%s-B33" % f for f in ("plain", "res", "res-rdrop", "keep", "res+keep", "one-launch")}
    keep |= {"metrics-cumulative-B257", "adam-3-steps", "adam-fused-equals-apply", "mixconv-structural-zeros", "replay-routeB", "replay-graph"}
    out = [c for c in plan(path) if c["id"] in keep or c["kind"] == "metric-edge"]
    missing = keep - {c["id"] for c in out}
    assert not missing, sorted(missing)
    return out


def describe(case):
    return "%s: %s engine, %s, T %d B %d grid_head %s options %s mode %s weights %s steps %d graphs %d" % (
        case["id"], case["engine"], {k: v for k, v in case["flags"].items() if mo.MIXEDNET_DEFAULTS.get(k) != v}, case["T"], case["B"],
        case["grid_head"], case["options"], case["mode"], case["weights"], case["steps"], case["graphs"])


# ------------------------------------------------------------------------------------------ models and batches
def case_layout(case):
    from microwakeword_amd.layout import GraphMixedNetLayout, MixedNetLayout
    return (GraphMixedNetLayout if case["engine"] == "graph" else MixedNetLayout)(case["flags"], case["T"])


def case_oracle(case):
    """The float64 oracle of the case's model: perturbed_oracle's scaling of the biases and BN parameters, and a dense kernel of
    random signs with magnitudes in [0.5, 1] x 2 / sqrt(n) - logits of order 1, and no final frame row whose terms all hide below
    the bound of z (the metric-edge cases: exact zeros and the case's bias)."""
    import engine_checks as ec
    om = ec.perturbed_oracle(case["T"], seed=case["seed"], flags=case["flags"])
    ws = om.get_weights()
    rng = np.random.default_rng(case["seed"] + 7)
    n = ws[-2].size
    kern = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.5, 1.0, size=n) * 2.0 / np.sqrt(n)
    bias = 0.05
    if case["kind"] == "metric-edge":
        kern, bias = np.zeros(n), case["bias"]
    ws[-2] = kern.astype(np.float32).reshape(ws[-2].shape)
    ws[-1] = np.array([bias], np.float32)
    om.set_weights(ws)
    return om


def case_batch(case, step=0, B=None):
    """x, y, w of step `step` (seeded by the case)."""
    import engine_checks as ec
    B = B or case["B"]
    rng = np.random.default_rng(1000 * case["seed"] + 17 * step + B)
    x = ec.synth_x(rng, B, case["T"])
    y = (rng.random(B) < 0.5).astype(np.float32)
    if case["kind"] == "metric-edge":
        y = (np.arange(B) % 2).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32)
    if case["weights"] == "zeros":
        w[::2] = 0.0
    return x, y, w


def case_keep(case, lay, step=0):
    """the explicit 0 / 1 dropout mask of a KEEP case"""
    rng = np.random.default_rng(case["seed"] + 31 + step)
    return (rng.random((case["B"], lay.t_last * lay.c_last)) >= case["dropout"]).astype(np.float32)


def input_condition(case):
    """The condition on a train case's inputs, from the float64 oracle alone: (frame rows that dropping would not show in z,
    windows that dropping would not show in the dense gradient) - both empty for a valid case.  None for the cases without a
    lost-row question (metric-edge: z is the bias by construction; partials: check_train_steps' own inputs; the Adam and
    structural-zero equalities)."""
    if case["kind"] not in ("train", "graph", "eval-metrics", "forward"):
        return None
    om = case_oracle(case)
    lay = case_layout(case)
    x, y, w = case_batch(case)
    taps = {}
    om.logits(x, case["mode"] == "train", taps=taps)
    last = [k for k in taps if k.endswith(".bn_out")][-1]
    a = np.maximum(taps[last].detach().numpy().astype(np.float64), 0.0)
    ws = om.get_weights()
    keep = None
    if case["dropout"] > 0:
        keep = case_keep(case, lay) / (1.0 - case["dropout"])
        a_head = a * keep.reshape(a.shape)
    else:
        a_head = a
    J = head_j(case["C"], a.shape[1]) if case["engine"] == "block" else -(-a.shape[1] * a.shape[2] // to.K_THREADS)
    h = to.head(a_head, ws[-2], ws[-1][0], y, w, J, clipped=case["options"].get("bce_from_logits", 1) == 0)
    rows = to.head_input_condition(h) if case["engine"] == "block" else np.zeros(0, int)
    if case["mode"] != "train":
        return rows, np.zeros(0, int)
    g = to.dense_grad(a, h["dz"].astype(np.float32), keep=keep)
    return rows, to.dense_input_condition(g, w != 0)


# ------------------------------------------------------------------------------------------ running a case
def _seg_offsets(lay):
    off, out = 0, {}
    for name, n in lay.segments():
        out[name] = (off, off + n)
        off += n
    return out


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound)) and np.all(np.isfinite(r))):   # a NaN / inf of the engine (or of a reference fed with one) is an error without bound
        return float("inf")
    return float(np.max(r)) if r.size else 0.0


def _finite(case, **values):
    """every value read back from the engine is finite (stale or uninitialised memory behind a clamped row shows as NaN first)"""
    for name, v in values.items():
        assert np.all(np.isfinite(np.asarray(v, np.float64))), "%s\nthe engine's %s holds a NaN / inf" % (describe(case), name)


class Ratios(dict):
    def add(self, name, err, bound):
        new = _ratio(err, bound)
        self[name] = new if not new <= self.get(name, 0.0) else self.get(name, 0.0)   # (keeps inf; max() would drop a NaN)

    def check(self, case):
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, "%s\nerror / derived bound above 1: %s\nall: %s" % (describe(case), bad, dict(self))


def _exact_metrics(eng, exact):
    """the engine's counters against oracle Metrics fed the engine's own probabilities: every integer exactly, bce_sum to 1e-12"""
    m = eng.metrics_raw()
    np.testing.assert_array_equal(np.array(m.hist101, np.float64).reshape(2, 101), exact.hist101)
    np.testing.assert_array_equal(np.array(m.hist200, np.float64).reshape(2, 200), exact.hist200)
    got = (m.n, m.correct, m.tp5, m.fp5, m.fn5, m.pos, m.neg)
    want = (exact.n, exact.correct, exact.tp5, exact.fp5, exact.fn5, exact.lab[1], exact.lab[0])
    assert tuple(float(v) for v in got) == tuple(float(v) for v in want), (got, want)
    # the sum is float64 on both sides, but metrics_body adds "(double)bce_value(...)": every term is a float32 value
    assert abs(m.bce_sum - exact.bce_sum) <= getattr(exact, "bce_tol", 0.0) + 1e-12 * max(1.0, abs(exact.bce_sum)), (m.bce_sum, exact.bce_sum, getattr(exact, "bce_tol", 0.0))


def _metrics_update(exact, pr, y, z, clipped):
    """oracle Metrics fed the engine's own probabilities / logits; exact.bce_tol collects the float32 rounding of the terms
    (tail_oracle.head: 4 * 2^-24 * (|z| + 1) in the logits form; 4 ulp of the value + the rounding of 1.0f - pc in the clipped one)"""
    exact.update(pr, y, None if clipped else z)
    if clipped:
        pc = np.clip(np.asarray(pr, np.float64), to.KERAS_LO, to.KERAS_HI)
        lab = np.asarray(y) > 0.5
        bce = -np.where(lab, np.log(pc), np.log(1 - pc))
        tol = 4 * to.U * np.abs(bce) + np.where(lab | (pc >= to.KERAS_HI), 0.0, to.U / (1 - pc))
    else:
        tol = 4 * to.U * (np.abs(np.asarray(z, np.float64)) + 1.0)
    exact.bce_tol = getattr(exact, "bce_tol", 0.0) + float(tol.sum())


def _make_engine(lib, case, lay, om, max_batch=None):
    from microwakeword_amd import native
    import engine_checks as ec
    B = max_batch or case["B"]
    if case["engine"] == "graph":
        eng = native.Engine(lib=lib, **dict(lay.engine_args(B), dropout=case["dropout"]))
        eng.set_grad_mask(lay.grad_mask())
        p, s = lay.pack(om.get_weights())
        eng.set_params(p)
        eng.set_bn_state(s)
    else:
        _, eng = ec.make_engine(lib, case["T"], B, om, flags=case["flags"])
    try:
        for k, v in case["options"].items():
            eng.set_option(k, v)
        if case["graphs"]:
            eng.set_option("graphs", 1)
    except Exception:
        eng.close()
        raise
    return eng


def grid_head_max(eng):
    """the largest accepted "grid_head" (4 x the device's CUs; the option table refuses more)"""
    from microwakeword_amd import native
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        try:
            eng.set_option("grid_head", mid)
            lo = mid
        except native.NativeError:
            hi = mid - 1
    eng.set_option("grid_head", lo)
    return lo


def _profile_names(eng):
    return [n for n, _ in eng.profile_read()]


_ROUTE_A = {}   # (library, T_final, B) -> (gradient, updated parameters) of route A, for the route-B case's bit comparison


def _run_train(lib, case, r):
    """Train steps (or one forward) of a block-engine case against the restatement."""
    lay, om = case_layout(case), case_oracle(case)
    B, C, nb = case["B"], case["C"], len(lay.blocks)
    eng = _make_engine(lib, case, lay, om, max_batch=None)
    try:
        grid = case["grid_head"]
        gmax = grid_head_max(eng)
        if grid < 0:
            grid = gmax
            B = grid + grid // 2
            eng.close()
            eng = _make_engine(lib, case, lay, om, max_batch=B)
        elif not grid:
            grid = gmax // 2   # mww_create's default: 2 x CUs
        eng.set_option("grid_head", grid)
        wpw = -(-B // min(B, grid))
        tf = lay.t_last
        J = head_j(C, tf)
        assert J is not None and tf == case.get("t_final", tf), (J, tf)
        clipped = case["options"].get("bce_from_logits", 1) == 0
        seg = _seg_offsets(lay)
        exact = mo.Metrics()
        mode = case["mode"]
        for step in range(case["steps"]):
            x, y, w = case_batch(case, step, B)
            p0 = eng.get_params()
            m0, v0, t0 = eng.get_opt_state()
            eng.set_batch(x)
            if mode != "forward":
                eng.set_targets(y, w)
            if mode == "train":
                eng.train_step(B, case["lrs"][step])
            else:
                eng.forward(B, training=False, update_metrics=(mode == "eval-metrics"))
            pr, z, loss = eng.read_outputs(B, want_loss=(mode == "train"))
            pL = eng.debug_read("p%d" % nb, B, B * tf * C).reshape(B, tf, C)
            bn = eng.debug_read("bn%d" % nb, B, 9 * C).reshape(9, C)
            wd, bd = p0[slice(*seg["dense.kernel"])], p0[seg["dense.bias"][0]]
            _finite(case, probabilities=pr, logits=z, loss=loss if mode == "train" else 0.0, p_L=pL, bn_rows=bn[:4])
            a, dec, _ = to.activations(pL, bn[0], bn[1])
            h = to.head(a, wd, bd, None if mode == "forward" else y, w, J, clipped=clipped)
            assert not len(to.head_input_condition(h)) or mode != "train", "the engine's own inputs miss the input condition"
            r.add("z", np.abs(z - h["z"]), h["bz"])
            r.add("p", np.abs(pr - h["p"]), h["bp"])
            if mode != "forward":
                _metrics_update(exact, pr, y, z, clipped)
                _exact_metrics(eng, exact)
            if mode != "train":
                continue
            dz = eng.debug_read("dz", B, B)
            r.add("loss", abs(loss - h["loss"]), h["bloss"])
            r.add("dz", np.abs(dz - h["dz"]), h["bdz"])
            assert np.all(dz[w == 0] == 0)
            g = eng.get_grads()
            _finite(case, dz=dz, gradient=g)
            dg = to.dense_grad(a, dz)
            r.add("dW_dense", np.abs(g[slice(*seg["dense.kernel"])] - dg["dW"]), dg["bW"])
            r.add("db_dense", abs(g[seg["dense.bias"][0]] - dg["db"]), dg["bdb"])
            bs = to.bn_sums(pL, bn[2], bn[3], dec, wd, dz, J, wpw)
            r.add("dgamma_L", np.abs(g[slice(*seg["b%d.bn.gamma" % (nb - 1)])] - bs["dgamma"]), bs["bdgamma"])
            r.add("dbeta_L", np.abs(g[slice(*seg["b%d.bn.beta" % (nb - 1)])] - bs["dbeta"]), bs["bdbeta"])
            p1 = eng.get_params()
            m1, v1, t1 = eng.get_opt_state()
            assert t1 == t0 + 1
            _finite(case, parameters=p1, adam_m=m1, adam_v=v1)
            pe, me, ve, bpar = to.adam_step(p0, m0, v0, g, case["lrs"][step], t1)
            r.add("adam_param", np.abs(p1 - pe), bpar)
            r.add("adam_m", np.abs(m1 - me), 4 * to.U * (np.abs(m0) + np.abs(g)))          # (g - m), the product, the sum
            r.add("adam_v", np.abs(v1 - ve), 4 * to.U * (np.abs(v0) + g.astype(np.float64) ** 2))
            if case.get("route") == "A":
                _ROUTE_A[(id(lib), tf, B)] = (g.copy(), p1.copy())
            if case.get("route") == "B":
                key = (id(lib), tf, B)
                if key not in _ROUTE_A:
                    ra = Ratios()
                    _run_train(lib, dict(case, options={}, route="A", expect=(), forbid=()), ra)
                ga, pa = _ROUTE_A[key]
                # kernels_tail.hip.h: "same arithmetic ... => bit-identical gradients either way"
                assert g.tobytes() == ga.tobytes(), "route A and route B gradients differ: %d elements" % int((g != ga).sum())
                assert p1.tobytes() == pa.tobytes(), "route A and route B updated parameters differ"
        if case["expect"] or case["forbid"]:
            # which launches ran: one more step under "profile" (event records around unchanged launches)
            eng.set_option("profile", 1)
            if mode == "train":
                eng.train_step(B, 1e-3)
            else:
                eng.forward(B, training=False, update_metrics=(mode == "eval-metrics"))
            eng.synchronize()
            names = _profile_names(eng)
            for n in case["expect"]:
                assert n in names, (n, names)
            for n in case["forbid"]:
                assert n not in names, (n, names)
    finally:
        eng.close()


def _run_graph(lib, case, r):
    """The graph engine's side work: dense_grad_kernel (or the one-launch form) and the metric update against the restatement,
    from the engine's own p_L, BN rows, residual branch, keep scale and dz."""
    from microwakeword_amd import native
    lay, om = case_layout(case), case_oracle(case)
    B, form = case["B"], case["form"]
    res, keep_on = form.startswith("res"), case["dropout"] > 0
    eng = _make_engine(lib, case, lay, om)
    try:
        n_ops = len(lay.ops)
        lo = lay.ops[-1]
        tf, C = lay.t_last, lay.c_last
        seg = _seg_offsets(lay)
        exact = mo.Metrics()
        for step in range(case["steps"]):
            x, y, w = case_batch(case, step)
            p0 = eng.get_params()
            m0, v0, t0 = eng.get_opt_state()
            eng.set_batch(x)
            eng.set_targets(y, w)
            if keep_on:
                eng.set_dropout_mask(case_keep(case, lay, step))
            eng.train_step(B, case["lrs"][step])
            pr, z, _ = eng.read_outputs(B)
            _metrics_update(exact, pr, y, z, False)
            _exact_metrics(eng, exact)
            pL = eng.debug_read("p%d" % n_ops, B, B * tf * C).reshape(B, tf, C)
            bn = eng.debug_read("bn%d" % n_ops, B, 9 * C).reshape(9, C)
            rs = None
            if res:
                ri, rdrop = lo["residual"], lo["residual_drop"]
                rT = lay.ops[ri]["tout"]
                rp = eng.debug_read("p%d" % (ri + 1), B, B * rT * C).reshape(B, rT, C)
                rbn = eng.debug_read("bn%d" % (ri + 1), B, 9 * C).reshape(9, C)
                assert rdrop == (0 if form == "res" else 2) and rT == tf + rdrop
                rs = (rp[:, rdrop:rdrop + tf], rbn[0], rbn[1])
            a, _, slack = to.activations(pL, bn[0], bn[1], res=rs)
            keep = None
            if keep_on:
                keep = eng.debug_read("keep", B, B * tf * C).reshape(B, tf * C)
                want = case_keep(case, lay, step) / np.float32(1.0 - case["dropout"])
                assert np.abs(keep - want).max() <= 2 * to.U * want.max(), "keep scale"
            dz = eng.debug_read("dz", B, B)
            g = eng.get_grads()
            _finite(case, probabilities=pr, logits=z, p_L=pL, bn_rows=bn[:4], dz=dz, gradient=g)
            dg = to.dense_grad(a, dz, keep=keep, slack=slack if res else None)
            assert not len(to.dense_input_condition(dg, w != 0)), "the engine's own inputs miss the input condition"
            r.add("dW_dense", np.abs(g[slice(*seg["dense.kernel"])] - dg["dW"]), dg["bW"])
            r.add("db_dense", abs(g[seg["dense.bias"][0]] - dg["db"]), dg["bdb"])
            p1 = eng.get_params()
            m1, v1, t1 = eng.get_opt_state()
            _finite(case, parameters=p1, adam_m=m1, adam_v=v1)
            pe, me, ve, bpar = to.adam_step(p0, m0, v0, g, case["lrs"][step], t1)
            r.add("adam_param", np.abs(p1 - pe), bpar)
        # which launches ran.  "profile" itself moves the side work onto the main stream and, with the metric update, into the
        # one-launch form: the plain dense_grad_kernel is named by a step without the metric update
        eng.set_option("profile", 1)
        one = form == "one-launch"
        eng.train_step(B, 1e-3, flags=0 if one else native.STEP_NO_METRICS)
        eng.synchronize()
        names = _profile_names(eng)
        assert ("dense_grad+metrics" in names) == one and ("dense_grad" in names) == (not one), names
        finals = [n for n in names if n.startswith("grad_final")]
        assert len(finals) == (2 if case.get("two_finals") else 1), (finals, "segments of the assembly: see kMaxFinalSegments")
    finally:
        eng.close()


def _run_metric_edge(lib, case, r):
    """z = the dense bias exactly; the three metric workgroup forms in turn, counters exact against oracle Metrics."""
    lay, om = case_layout(case), case_oracle(case)
    B, bias = case["B"], np.float32(case["bias"])
    clipped = case["options"].get("bce_from_logits", 1) == 0
    eng = _make_engine(lib, case, lay, om)
    try:
        p0 = eng.get_params()
        exact = mo.Metrics()
        x, y, w = case_batch(case)
        for form in ("grad_final", "head_tail", "metrics_kernel"):
            eng.set_params(p0)
            eng.set_option("tail_roles", 1 if form == "grad_final" else 0)
            eng.set_batch(x)
            eng.set_targets(y, w)
            if form == "metrics_kernel":
                eng.forward(B, training=False, update_metrics=True)
            else:
                eng.train_step(B, 1e-3)
            pr, z, loss = eng.read_outputs(B, want_loss=form != "metrics_kernel")
            assert np.all(z == bias), z
            want = {0.0: np.float32(0.5), 40.0: np.float32(1.0), -110.0: np.float32(0.0)}.get(float(bias))
            if want is not None:
                assert np.all(pr == want), pr
            else:
                assert np.all((pr > 0) & (pr < 1e-17)), pr
            if form != "metrics_kernel":
                assert np.isfinite(loss)
                if not clipped or bias == 0:   # (the clipped form of a saturated p sits on the clip itself: finite is all that is asked)
                    ref = to.head(np.zeros((B, 1, 1)), np.zeros(1), float(bias), y, w, 2, clipped=clipped)
                    r.add("loss", abs(loss - ref["loss"]), ref["bloss"] + 4 * to.U * abs(ref["loss"]))
            _metrics_update(exact, pr, y, z, clipped)
            _exact_metrics(eng, exact)
        m = eng.metrics_raw()
        b101 = {0.0: 49, 40.0: 99, -40.0: 0}.get(float(bias))   # ceil(p * 100) - 1; p == 0 has no hist101 bucket
        h101 = np.array(m.hist101, np.int64).reshape(2, 101)
        assert h101.sum() == (0 if b101 is None else 3 * B) and (b101 is None or h101[:, b101].sum() == 3 * B), h101
        b200 = {0.0: 99, 40.0: 198, -40.0: 0, -110.0: 0}[float(bias)]
        assert np.array(m.hist200, np.int64).reshape(2, 200)[:, b200].sum() == 3 * B
    finally:
        eng.close()


def _run_cumulative(lib, case, r):
    """One accumulation across the three metric workgroup forms and varying B, with a reset in the middle."""
    lay, om = case_layout(case), case_oracle(case)
    eng, fresh = _make_engine(lib, case, lay, om), _make_engine(lib, case, lay, om)
    try:
        p0, s0 = eng.get_params(), eng.get_bn_state()
        exact = mo.Metrics()
        mid, big = case["sizes"]
        seq = (("grad_final", 1), ("head_tail", 63), ("metrics_kernel", mid), ("grad_final", big), ("reset", 0), ("metrics_kernel", 63),
               ("head_tail", big), ("grad_final", mid), ("metrics_kernel", 1), ("head_tail", 1), ("metrics_kernel", big))
        total, bce_ref = 0, 0.0
        for k, (form, B) in enumerate(seq):
            if form == "reset":
                eng.metrics_reset()
                exact.reset()
                exact.bce_tol = 0.0
                total, bce_ref = 0, 0.0
                _exact_metrics(eng, exact)
                continue
            x, y, w = case_batch(case, k, B)
            fresh.metrics_reset()
            for e in (eng, fresh):   # `fresh` starts every batch from zero: the increment of this batch alone
                e.set_params(p0)
                e.set_bn_state(s0)
                e.set_option("tail_roles", 1 if form == "grad_final" else 0)
                e.set_batch(x)
                e.set_targets(y, w)
                if form == "metrics_kernel":
                    e.forward(B, training=False, update_metrics=True)
                else:
                    e.train_step(B, 1e-3)
            pr, z, _ = eng.read_outputs(B, want_loss=False)
            _metrics_update(exact, pr, y, z, False)
            total += B
            _exact_metrics(eng, exact)
            got = eng.metrics_raw()
            assert got.n == total
            # the accumulation itself is float64 on both sides, only the order differs: the engine's own increments, summed
            bce_ref += fresh.metrics_raw().bce_sum
            assert abs(got.bce_sum - bce_ref) <= 1e-12 * max(1.0, abs(bce_ref)), (got.bce_sum, bce_ref)
    finally:
        eng.close()
        fresh.close()


def _run_adam_apply(lib, case, r):
    """The fused grad_final+adam route is bit-identical to STEP_NO_APPLY + apply_gradients (adam_kernel)."""
    from microwakeword_amd import native
    lay, om = case_layout(case), case_oracle(case)
    a, b = _make_engine(lib, case, lay, om), _make_engine(lib, case, lay, om)
    try:
        for step in range(case["steps"]):
            x, y, w = case_batch(case, step)
            for eng in (a, b):
                eng.set_batch(x)
                eng.set_targets(y, w)
            a.train_step(case["B"], case["lrs"][step])
            b.train_step(case["B"], case["lrs"][step], flags=native.STEP_NO_APPLY)
            b.apply_gradients(case["lrs"][step])
            assert a.get_grads().tobytes() == b.get_grads().tobytes()
            assert a.get_params().tobytes() == b.get_params().tobytes(), step
            (ma, va, ta), (mb, vb, tb) = a.get_opt_state(), b.get_opt_state()
            assert ma.tobytes() == mb.tobytes() and va.tobytes() == vb.tobytes() and ta == tb == step + 1
        b.set_option("profile", 1)
        b.apply_gradients(1e-3)
        b.synchronize()
        assert "adam" in _profile_names(b)
    finally:
        a.close()
        b.close()


def _run_mixconv(lib, case, r):
    """Structural zeros of a MixConv with unequal groups: gradient exactly 0, parameter and both Adam slots bit-unchanged."""
    lay, om = case_layout(case), case_oracle(case)
    eng = _make_engine(lib, case, lay, om)
    try:
        zero = lay.grad_mask() == 0
        assert zero.sum() == 2 * 16, zero.sum()   # the 3-tap group of 16 channels inside the fused 5-tap table
        p0 = eng.get_params()
        assert np.all(p0[zero] == 0)
        for step in range(case["steps"]):
            x, y, w = case_batch(case, step)
            eng.set_batch(x)
            eng.set_targets(y, w)
            eng.train_step(case["B"], case["lrs"][step])
            g = eng.get_grads()
            assert np.all(g[zero] == 0) and np.abs(g[~zero]).max() > 0
        m, v, t = eng.get_opt_state()
        assert t == case["steps"]
        assert eng.get_params()[zero].tobytes() == p0[zero].tobytes()
        assert m[zero].tobytes() == np.zeros(int(zero.sum()), np.float32).tobytes() == v[zero].tobytes()
        assert np.all(v[~zero] >= 0) and np.count_nonzero(m[~zero]) > 0.5 * (~zero).sum()
    finally:
        eng.close()


def _run_graph_whole_step(lib, case, r):
    """engine_checks.check_graph_mixednet, unchanged and strict (no unit of this case sits at a ReLU zero: asserted)"""
    import engine_checks as ec
    assert ec.count_graph_mixednet_near_zero(case["flags"], case["B"], case["T"], steps=1, seed=case["seed"]) == 0
    ec.check_graph_mixednet(lib, case["flags"], B=case["B"], T=case["T"], steps=1, grid=0, seed=case["seed"], strict=True)


def _run_partials(lib, case, r):
    import engine_checks as ec
    ec.check_train_steps(lib, B=case["B"], T=case["T"], steps=1, grid=case["grid"], flags=case["flags"])


_RUNNERS = {"train": _run_train, "eval-metrics": _run_train, "forward": _run_train, "graph": _run_graph, "metric-edge": _run_metric_edge,
            "cumulative": _run_cumulative, "graph-whole-step": _run_graph_whole_step, "adam-apply": _run_adam_apply, "mixconv": _run_mixconv, "partials": _run_partials}


def run_case(lib, case):
    """Runs the case; returns {quantity: worst error / derived bound} (and prints it, one line per case, before asserting)."""
    r = Ratios()
    try:
        _RUNNERS[case["kind"]](lib, case, r)
    finally:
        print("TAIL-SWEEP %s %s" % (case["id"], " ".join("%s=%.3f" % kv for kv in sorted(r.items()))), flush=True)
    r.check(case)
    return r
