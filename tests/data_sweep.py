"""A covering sweep of every reader of window descriptors (``mww_window``: store id, pad_rows, copy_rows, 64-bit src_elem, plus
SpecAugment (start, width) masks) at the edges of the descriptors and of the masks, shared by the GPU sweep
(tests/test_data_sweep_gpu.py) and its CPU-side checks (tests/test_data_sweep_emulated.py).  The manner of tests/tail_sweep.py
and tests/graph_table_sweep.py.  The readers:

- ``assemble_kernel`` (csrc/kernels_data.hip.h) writes the materialised batch;
- ``xgather_setup`` / ``XStage::issue`` / ``commit`` / ``commit_planes`` (kernels_fwd.hip.h), the "fused_input" gather inside
  fwd_first_kernel, bwd_first_kernel and bwd_firstw_kernel (fp32, the bf16 modes, x6);
- ``gx_setup`` ... ``gx_commit`` (kernels_graph.hip.h), the gathering stem gconv_xg_kernel / gconv_wgrad_xg_kernel;
- ``mww_evaluate_windows`` / ``mww_bn_reestimate_windows`` over whole window lists;
- ``frame_value`` (stream_common.hip.h) of the float, int8, graph, graph-int8 and calibration streaming kernels;
- ``mine_clip`` (tu_stream_mine.hip), which emits descriptors.

Descriptors and masks are WRITTEN by the plan, not drawn by the sampler: that is how store id 63, ``copy_rows == 0`` and masks
at chosen bit positions are reached.  ``required()`` lists the axis items, ``plan()`` is a deterministic list of small cases built
without a GPU, ``case_items(case)`` DERIVES what a case covers from its descriptors, masks, grids and options (the stream, list
and large-store cases name theirs), ``uncovered()`` must be empty, ``run_case(lib, case)`` runs one case.

Every comparison is exact (bits through a uint32 view, so -0.0, denormals and NaN payloads count):

1. the batch ``get_batch`` returns under "fused_input" 0 against ``oracle/data_oracle.materialise`` of the same descriptor;
2. evaluation logits, ``debug_read("a0")`` (block engine outside "storage_bf16"), the flat gradient, probabilities and loss of a
   ``STEP_NO_APPLY`` train step between "fused_input" 1 and 0 on the same random model (``perturbed_oracle``) and descriptors;
3. the route: under "profile" the names from the assembly call to the end of the step hold no ``assemble`` launch where the case
   is declared "gather" and exactly one where it is declared "materialised"; graph-engine cases also hold the launch names to
   ``graph_table_sweep.case_route`` and name the XG instantiations (``graph_table_sweep.case_kernels``);
4. observability, host-only: for every window the reference of each neighbouring WRONG descriptor - pad_rows +-1, src_elem +-40,
   each mask start +-1 and width +-1, the other dtype, the neighbouring store - differs from the right one.  A neighbour the ABI
   refuses (a negative pad, a read past the store) is no wrong descriptor a kernel could be handed and is skipped; so is one that
   names the SAME cells of the same store (``symbolic()``: e.g. the width of a mask that already runs past T, one of two
   identical masks, src_elem of a window that copies no row) - no data could tell those apart.  Every other neighbour must show
   in the data: all store values of the model-route cases are finite and nonzero (uint16 in 1..666, float32 in (0, 26]).

Items (the terms of required()):
  ("copy_rows", "0" | "1" | "T-1" | "T"), ("src_elem", 0), ("ends-on-last-element",), ("store-is-one-window",)
  ("dtype", "u16-alone" | "f32-alone" | "mixed-batch" | "mixed-workgroup"), ("store", 0 | 1 | 62 | 63)
  ("value", name)                           materialised route: u16 0 / 1 / 65535, f32 -0.0 / denormal / FLT_MAX, NaN and +-inf
                                            under a mask (-> +0.0) and outside one (bits kept)
  ("masks", route, ntm, nfm)                route "gather" | "materialised" | "refused"
  ("tmask", name), ("fmask", name)          counted on gather-route cases only (the bitmaps of xgather_setup / gx_setup)
  ("T", ...)                                the window lengths at which a route or a tile count changes
  ("per-wg", engine, B, grids..., route), ("eight-distinct-windows",)
  ("form", name)                            the kernel forms that stage x
  ("split", T, n), ("split-refused",), ("targets",), ("window-list", ...), ("stream", ...), ("large-store",)"""
import functools
import os
import re

import numpy as np

import block_table_sweep as bts
import graph_table_sweep as gs
from oracle import data_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "microwakeword_amd", "csrc")
SEED = 2026
BINS = 40

# limits the plan mirrors (tests/test_data_sweep_emulated.py holds them to the headers: header_constants())
K_XMAX_SAMPLES = 8     # kXMaxSamples: windows per workgroup the gather keeps descriptors for
K_XROW_WORDS = 8       # kXRowWords: 32-frame words of the row bitmap
K_XMAX_MASKS = 8       # kXMaxMasks: masks per window in gather mode
K_MAX_MASKS = 16       # kMaxMasks: masks per window the assembly kernel takes
K_GXROWS = 200         # kGXRows: frames of a window the graph stem gathers
MAX_STORES = 64        # MWW_MAX_STORES
SPLIT_RANGE = (1, 8)   # "assemble_split"
T_BITMAP = 32 * K_XROW_WORDS

# first blocks (K1, C1, CO, K, S) of the two block-engine models: engine_checks.DEF and .NOTEBOOK (a strided first block of
# block_table_sweep's table; the emulated test asserts it is one)
FIRST = {"DEF": (3, 32, 48, 5, 1), "STRIDED": (5, 32, 64, 5, 3)}
T_MIN = 47             # the smallest window engine_checks.DEF accepts
SPLITS = (1, 2, 3, 5, 7, 8)


def header_constants():
    """The limits as the sources state them."""
    def grab(path, pattern):
        m = re.search(pattern, open(path).read())
        if not m:
            raise ValueError("cannot parse %s for %s" % (path, pattern))
        return tuple(int(g) for g in m.groups()) if len(m.groups()) > 1 else int(m.group(1))
    fwd, data, graph = (os.path.join(CSRC, n) for n in ("kernels_fwd.hip.h", "kernels_data.hip.h", "kernels_graph.hip.h"))
    return dict(K_XMAX_SAMPLES=grab(fwd, r"constexpr int kXMaxSamples = (\d+);"), K_XROW_WORDS=grab(fwd, r"constexpr int kXRowWords = (\d+);"),
                K_XMAX_MASKS=grab(fwd, r"constexpr int kXMaxMasks = (\d+);"), K_MAX_MASKS=grab(data, r"constexpr int kMaxMasks = (\d+);"),
                K_GXROWS=grab(graph, r"constexpr int kGXRows = (\d+);"),
                MAX_STORES=grab(os.path.join(ROOT, "include", "mww.h"), r"#define MWW_MAX_STORES (\d+)"),
                SPLIT_RANGE=grab(os.path.join(CSRC, "mww_lib.hip"), r'\{"assemble_split", OPT_CORE, (\d+), (\d+), 0,'))


# ------------------------------------------------------------------------------------------ stores and references
def build_store(spec):
    """The flat array of a store spec (id, dtype, rows, seed, poke): every value finite and nonzero - uint16 in 1..666, float32 in
    (0, 26] - except the elements a values case pokes in as bits."""
    sid, dtype, rows, seed, poke = spec
    rng = np.random.default_rng([SEED, seed, sid])
    n = rows * BINS
    if dtype == "u16":
        a = rng.integers(1, 667, size=n, dtype=np.uint16)
    else:
        a = ((1.0 - rng.random(n)) * 26.0).astype(np.float32)
        assert a.min() > 0 and a.max() <= 26
    for row, f, bits in poke:
        a.view(np.uint16 if dtype == "u16" else np.uint32)[row * BINS + f] = bits
    return a


def build_stores(case):
    return {spec[0]: build_store(spec) for spec in case["stores"]}


def window_masks(case, i):
    m = case["masks"][i]
    return [tuple(p) for p in m[:case["ntm"]]], [tuple(p) for p in m[case["ntm"]:]]


def reference(store, w, tm, fm, T):
    """oracle/data_oracle.materialise of window w = (store id, pad_rows, copy_rows, src_elem) of the flat ``store``."""
    _, pad, copy, src = w
    assert pad + copy == T and src % BINS == 0
    d = do.WindowDesc(provider=0, store=0, sample=0, src_row=0, copy_rows=copy, pad_rows=pad, time_masks=list(tm), freq_masks=list(fm))
    out = do.materialise(store[src:src + copy * BINS].reshape(copy, BINS), d, T)   # (the sample: the rows the window names)
    assert out.shape == (T, BINS) and out.dtype == np.float32
    return out


def reference_batch(case, stores):
    return np.stack([reference(stores[w[0]], w, *window_masks(case, i), case["T"]) for i, w in enumerate(case["windows"])])


def symbolic(w, tm, fm, T):
    """Which store element every output cell is: int64 [T, 40], -1 for a cell that is zero whatever the store holds."""
    _, pad, copy, src = w
    out = np.full((T, BINS), -1, np.int64)
    out[pad:pad + copy] = src + np.arange(copy * BINS, dtype=np.int64).reshape(copy, BINS)
    for t0, t in tm:
        out[t0:t0 + t, :] = -1
    for f0, f in fm:
        out[:, f0:f0 + f] = -1
    return out


def _valid(w, n_elems, T):
    _, pad, copy, src = w
    return pad >= 0 and copy >= 0 and pad + copy == T and src >= 0 and src + copy * BINS <= n_elems


def neighbours(case, stores, i):
    """(name, flat store, window, time masks, freq masks) of every neighbouring wrong descriptor of window i the ABI accepts."""
    T = case["T"]
    w = tuple(case["windows"][i])
    sid, pad, copy, src = w
    tm, fm = window_masks(case, i)
    st = stores[sid]
    out = []
    for d in (-1, 1):
        out.append(("pad_rows%+d" % d, st, (sid, pad + d, copy - d, src), tm, fm))
        out.append(("src_elem%+d" % (BINS * d), st, (sid, pad, copy, src + BINS * d), tm, fm))
        for kind, ms in (("t", tm), ("f", fm)):
            for k, (s0, wd) in enumerate(ms):
                for name, m in (("start", (s0 + d, wd)), ("width", (s0, wd + d))):
                    if m[0] < 0 or m[1] < 0:
                        continue
                    ms2 = list(ms)
                    ms2[k] = m
                    out.append(("%smask%d.%s%+d" % (kind, k, name, d), st, w, ms2 if kind == "t" else tm, ms2 if kind == "f" else fm))
    out.append(("other dtype", st.view(np.float32 if st.dtype == np.uint16 else np.uint16), w, tm, fm))
    if sid ^ 1 in stores:
        out.append(("store %d" % (sid ^ 1), stores[sid ^ 1], (sid ^ 1, pad, copy, src), tm, fm))
    return [(name, s, w2, a, b) for name, s, w2, a, b in out if _valid(w2, s.size, T)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_observability(case, stores, ref):
    """Comparison 4 of the module docstring.  Returns the number of neighbours that had to show and did."""
    T, shown = case["T"], 0
    for i, w in enumerate(case["windows"]):
        tm, fm = window_masks(case, i)
        sym = symbolic(w, tm, fm, T)
        for name, st, w2, tm2, fm2 in neighbours(case, stores, i):
            sym2 = symbolic(w2, tm2, fm2, T)
            same_source = st is stores[w[0]] or not (sym >= 0).any()
            if same_source and np.array_equal(sym, sym2):
                continue   # the same cells of the same store: the same batch by construction
            assert not same_bits(reference(st, w2, tm2, fm2, T), ref[i]), "%s: window %d %s cannot show a wrong %s" % (case["id"], i, w, name)
            shown += 1
    return shown


# ------------------------------------------------------------------------------------------ items
TMASKS = ("[0,1)", "[T-1,T)", "[31,33)", "[32,64)", "[30,100)", "[0,T)", "width-0", "overlapping", "identical", "past-T", "T256:[224,256)", "T256:[255,256)")
FMASKS = ("[0,1)", "[39,40)", "[3,5)", "[2,7)", "[31,33)", "[28,36)", "[32,40)", "[0,40)", "width-0", "past-40", "crossing")
VALUES = ("u16-0", "u16-1", "u16-65535", "f32-neg-zero", "f32-denormal", "f32-max", "nan-masked", "nan-kept", "+inf-masked", "+inf-kept",
          "-inf-masked", "-inf-kept")
FORMS = ("fwd_first-plain", "fwd_first-x6", "bwd_first-plain", "bwd_first-x6", "bwd_firstw-strided", "bwd_firstw-x6", "pointwise_bf16",
         "storage_bf16", "gconv_xg_kernel", "gconv_wgrad_xg_kernel")


def required():
    req = [("copy_rows", n) for n in ("0", "1", "T-1", "T")] + [("src_elem", 0), ("ends-on-last-element",), ("store-is-one-window",)]
    req += [("dtype", n) for n in ("u16-alone", "f32-alone", "mixed-batch", "mixed-workgroup")]
    req += [("store", s) for s in (0, 1, MAX_STORES - 2, MAX_STORES - 1)]
    req += [("value", n) for n in VALUES]
    req += [("masks", "gather", a, b) for a, b in ((0, 0), (1, 0), (0, 1), (K_XMAX_MASKS, 0), (0, K_XMAX_MASKS), (K_XMAX_MASKS // 2, K_XMAX_MASKS // 2))]
    req += [("masks", "materialised", a, b) for a, b in ((K_XMAX_MASKS // 2 + 1, K_XMAX_MASKS // 2), (K_MAX_MASKS, 0), (0, K_MAX_MASKS),
                                                         (K_MAX_MASKS // 2, K_MAX_MASKS // 2))]
    req += [("masks", "refused", K_MAX_MASKS // 2 + 1, K_MAX_MASKS // 2)]
    req += [("tmask", n) for n in TMASKS] + [("fmask", n) for n in FMASKS]
    req += [("T", "block", T_BITMAP, "gather"), ("T", "block", T_BITMAP + 1, "materialised")]
    req += [("T", "stride1", n) for n in ("one-tile", "one-tile+1", "two-tiles+1")] + [("T", "strided", n) for n in ("tail", "two-tile", "remainder")]
    req += [("T", "graph", K_GXROWS - 1, "gather"), ("T", "graph", K_GXROWS, "gather"), ("T", "graph", K_GXROWS + 1, "materialised")]
    two = 2 * K_XMAX_SAMPLES
    req += [("per-wg", "block", 2, 2, 2, "gather"), ("per-wg", "block", 5, 2, 2, "gather"), ("per-wg", "block", two, 2, 2, "gather"),
            ("per-wg", "block", two + 1, 2, 2, "materialised"), ("per-wg", "block", two + 1, 4, 2, "materialised"),
            ("per-wg", "graph", two, 2, "gather"), ("per-wg", "graph", two + 1, 2, "materialised"), ("eight-distinct-windows",)]
    req += [("form", n) for n in FORMS]
    req += [("split", T, n) for T in (194, T_MIN) for n in SPLITS] + [("split-refused",)]
    req += [("targets",), ("window-list", "evaluate", "n%batch"), ("window-list", "evaluate", "n<batch"), ("window-list", "bn_reestimate")]
    req += [("stream", n) for n in ("float", "int8", "graph", "graph-int8", "calibrate", "mine")]
    req += [("large-store",)]
    assert len(set(req)) == len(req)
    return req


def mode_of(case):
    return 2 if case["options"].get("st_bf16") else (1 if case["options"].get("pw_bf16") else 0)


def form_options(case):
    return {k: v for k, v in case["options"].items() if k in bts.OPTION_DEFAULTS}


def graph_case(case, lazy):
    """The case as graph_table_sweep sees it: kind "gather" = a descriptor-only batch."""
    import engine_checks as ec
    return gs._case(case["id"], "gather" if lazy else "inception", ec.INC, case["T"], len(case["windows"]), case["grids"].get("grid_graph", 0))


def workgroups(case):
    """The window indices of every gathering workgroup (xgather_setup: window blockIdx.x + s * gridDim.x), per launch grid."""
    B = len(case["windows"])
    names = ("grid_graph",) if case["model"] == "INC" else ("grid_fwd", "grid_bwd")
    out = []
    for n in names:
        g = case["grids"].get(n, 0)
        g = min(B, g) if g > 0 else B   # (the automatic grids give every window of these small batches a workgroup)
        out += [list(range(b, B, g)) for b in range(g)]
    return out


def expected_route(case):
    """The route the host conditions give a "fused_input" 1 batch of the case (mww_assemble_batch, BlockModel::lazy_ok,
    g_stem_gathers and launch_gconv / launch_gwgrad), restated."""
    T, nm = case["T"], case["ntm"] + case["nfm"]
    per = max(len(g) for g in workgroups(case))
    if case["model"] == "INC":
        ok = T <= K_GXROWS and T <= T_BITMAP and nm <= K_XMAX_MASKS and per <= K_XMAX_SAMPLES
    else:
        ok = T <= T_BITMAP and nm <= K_XMAX_MASKS and per <= K_XMAX_SAMPLES
    return "gather" if ok else "materialised"


def _mask_items(case):
    T, items = case["T"], set()
    for i, w in enumerate(case["windows"]):
        tm, fm = window_masks(case, i)
        for s, wd in tm:
            for name, m in (("[0,1)", (0, 1)), ("[T-1,T)", (T - 1, 1)), ("[31,33)", (31, 2)), ("[32,64)", (32, 32)), ("[30,100)", (30, 70)), ("[0,T)", (0, T))):
                if (s, wd) == m and s + wd <= T:
                    items.add(("tmask", name))
            if wd == 0:
                items.add(("tmask", "width-0"))
            if s < T < s + wd:
                items.add(("tmask", "past-T"))
            if T == T_BITMAP and (s, wd) in ((T - 32, 32), (T - 1, 1)):
                items.add(("tmask", "T256:[%d,256)" % s))
        for a in range(len(tm)):
            for b in range(a + 1, len(tm)):
                (s0, w0), (s1, w1) = tm[a], tm[b]
                if w0 > 0 and w1 > 0 and tm[a] == tm[b]:
                    items.add(("tmask", "identical"))
                elif w0 > 0 and w1 > 0 and max(s0, s1) < min(s0 + w0, s1 + w1):
                    items.add(("tmask", "overlapping"))
        for s, wd in fm:
            for name, m in (("[0,1)", (0, 1)), ("[39,40)", (39, 1)), ("[3,5)", (3, 2)), ("[2,7)", (2, 5)), ("[31,33)", (31, 2)), ("[28,36)", (28, 8)),
                            ("[32,40)", (32, 8)), ("[0,40)", (0, 40))):
                if (s, wd) == m:
                    items.add(("fmask", name))
            if wd == 0:
                items.add(("fmask", "width-0"))
            if s < BINS < s + wd:
                items.add(("fmask", "past-40"))
        pad = w[1]
        if any(wd > 0 and s + wd > pad and s < T for s, wd in tm) and any(wd > 0 and s < BINS for s, wd in fm) and w[2] > 0:
            items.add(("fmask", "crossing"))   # a data row under a time mask that a frequency mask crosses
    return items


def case_items(case):
    """What a case covers (the terms of required())."""
    items = set(tuple(i) for i in case["items"])
    kind = case["kind"]
    if kind not in ("route", "batch"):
        return items
    T, B, wins = case["T"], len(case["windows"]), case["windows"]
    rows = {s[0]: s[2] for s in case["stores"]}
    dt = {s[0]: s[1] for s in case["stores"]}
    gather = kind == "route" and case["route"] == "gather"
    if kind == "route":
        items.add(("masks", case["route"], case["ntm"], case["nfm"]))
    if kind == "batch" and case["split"] is not None:
        items.add(("split", T, case["split"]))
    if not gather:
        if kind == "route":
            if case["model"] == "INC":
                if case["grids"].get("grid_graph", 0):
                    items.add(("per-wg", "graph", B, case["grids"]["grid_graph"], "materialised"))
                if T > K_GXROWS:
                    items.add(("T", "graph", T, "materialised"))
            else:
                if "grid_fwd" in case["grids"]:
                    items.add(("per-wg", "block", B, case["grids"]["grid_fwd"], case["grids"]["grid_bwd"], "materialised"))
                if T > T_BITMAP:
                    items.add(("T", "block", T, "materialised"))
        return items
    # ---- a gathering case: the descriptors, dtypes, stores, masks, tiles, workgroups and kernel forms it takes through the gather
    for sid, pad, copy, src in wins:
        for name, n in (("0", 0), ("1", 1), ("T-1", T - 1), ("T", T)):
            if copy == n:
                items.add(("copy_rows", name))
        if src == 0 and copy > 0:
            items.add(("src_elem", 0))
        if copy > 0 and src + copy * BINS == rows[sid] * BINS:
            items.add(("ends-on-last-element",))
        if copy == T and rows[sid] == T:
            items.add(("store-is-one-window",))
        if copy > 0 and sid in (0, 1, MAX_STORES - 2, MAX_STORES - 1) and sid ^ 1 in rows:
            items.add(("store", sid))
    used = {dt[w[0]] for w in wins}
    items.add(("dtype", "mixed-batch") if len(used) == 2 else ("dtype", "%s-alone" % used.pop()))
    groups = workgroups(case)
    if all(len({dt[wins[i][0]] for i in g if wins[i][2] > 0}) == 2 for g in groups):
        items.add(("dtype", "mixed-workgroup"))
    items |= _mask_items(case)
    if case["model"] == "INC":
        items.add(("T", "graph", T, "gather"))
        if case["grids"].get("grid_graph", 0):
            items.add(("per-wg", "graph", B, case["grids"]["grid_graph"], "gather"))
        for k in gs.case_kernels(graph_case(case, True)):
            if "_xg_kernel" in k:
                items.add(("form", k.split("<")[0]))
    else:
        k1, _, _, k, s = FIRST[case["model"]]
        ta = (T - k1) // s + 1
        if T == T_BITMAP:
            items.add(("T", "block", T, "gather"))
        if s == 1:
            for name, n in (("one-tile", bts.TT), ("one-tile+1", bts.TT + 1), ("two-tiles+1", 2 * bts.TT + 1)):
                if ta == n:
                    items.add(("T", "stride1", name))
        else:
            tmode = bts.tile_mode(FIRST[case["model"]], T)
            if tmode != "one":
                items.add(("T", "strided", tmode))
            if (T - k1) % s != 0 and tmode == "two-tile":
                items.add(("T", "strided", "remainder"))
        if "grid_fwd" in case["grids"]:
            items.add(("per-wg", "block", B, case["grids"]["grid_fwd"], case["grids"]["grid_bwd"], "gather"))
        mode, o = mode_of(case), form_options(case)
        fwd = bts.instantiation("fwd_first", FIRST[case["model"]], mode, o)
        bwd = bts.instantiation("bwd_first", FIRST[case["model"]], mode, o)
        if mode == 0:
            items.add(("form", "fwd_first-" + ("x6" if bts._form_tag(fwd) == "x6" else "plain")))
            items.add(("form", {"narrow": "bwd_first-plain", "narrow-x6": "bwd_first-x6", "wide": "bwd_firstw-strided", "wide-x6": "bwd_firstw-x6"}[bts._form_tag(bwd)]))
        else:
            items.add(("form", "pointwise_bf16" if mode == 1 else "storage_bf16"))
    for g in groups:
        if len(g) == K_XMAX_SAMPLES:
            own = [wins[i] for i in g]
            ms = [tuple(map(tuple, case["masks"][i])) for i in g]
            if (len({w[1] for w in own}) == len(g) and len({dt[w[0]] for w in own}) == 2 and len({w[0] for w in own}) >= 2
                    and len(set(ms)) == len(g) and case["ntm"] + case["nfm"] > 0):
                items.add(("eight-distinct-windows",))
    return items


# ------------------------------------------------------------------------------------------ plan
def _case(cid, kind, model="DEF", T=T_MIN, stores=(), windows=(), ntm=0, nfm=0, masks=None, route=None, options=None, grids=None,
          split=None, items=(), gpu_only=False, **extra):
    B = len(windows)
    masks = masks if masks is not None else [[(0, 0)] * (ntm + nfm) for _ in range(B)]
    assert len(masks) == B and all(len(m) == ntm + nfm for m in masks), cid
    c = dict(id=cid, kind=kind, model=model, T=int(T), stores=[tuple(s) for s in stores], windows=[tuple(int(v) for v in w) for w in windows],
             ntm=int(ntm), nfm=int(nfm), masks=[[tuple(int(v) for v in p) for p in m] for m in masks], route=route,
             options=dict(options or {}), grids=dict(grids or {}), split=split, items=[tuple(i) for i in items], gpu_only=bool(gpu_only))
    c.update(extra)
    return c


def std_stores(T, extra=20, seed=0):
    """Four stores whose neighbouring ids (0 / 1, 62 / 63) hold different data of different dtypes."""
    return [(0, "u16", T + extra, seed, ()), (1, "f32", T + extra, seed, ()), (MAX_STORES - 2, "f32", T + extra, seed + 1, ()),
            (MAX_STORES - 1, "u16", T + extra, seed + 1, ())]


_STORE_ORDER = (0, 1, 1, 0, MAX_STORES - 1, MAX_STORES - 2, MAX_STORES - 2, MAX_STORES - 1)


def std_windows(T, B, extra=20):
    """B windows over std_stores: with two workgroups either one owns both dtypes and all four stores; the pads differ within a
    workgroup of eight."""
    pads = [0, 3, 1, T // 2, 7, 0, T - 2, 2, 5, 11, 9, 1, 13, 4, 21, 6, 17]
    out = []
    for i in range(B):
        pad = pads[i % len(pads)]
        copy = T - pad
        out.append((_STORE_ORDER[i % 8], pad, copy, BINS * ((5 * i + 1) % (extra + pad + 1))))
    return out


def fill_masks(B, ntm, nfm, chosen):
    """[B][ntm + nfm] (start, width): ``chosen`` = {window: (time masks, frequency masks)}, completed with width-0 masks at
    scattered starts (what SpecAugment draws when the width comes out 0)."""
    out = []
    for i in range(B):
        tm, fm = chosen.get(i, ((), ()))
        tm, fm = list(tm), list(fm)
        assert len(tm) <= ntm and len(fm) <= nfm
        tm += [(7 + 3 * k + i, 0) for k in range(ntm - len(tm))]
        fm += [(2 + 5 * k + i, 0) for k in range(nfm - len(fm))]
        out.append(tm + fm)
    return out


def _route(cid, T, B, ntm=0, nfm=0, chosen=None, model="DEF", route="gather", options=None, grids=None, stores=None, windows=None, **kw):
    return _case(cid, "route", model=model, T=T, stores=stores if stores is not None else std_stores(T), windows=windows if windows is not None else std_windows(T, B),
                 ntm=ntm, nfm=nfm, masks=fill_masks(B, ntm, nfm, chosen or {}), route=route, options=options, grids=grids, **kw)


def _f32(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def _plan():
    P = []
    T = T_MIN
    G2 = dict(grid_fwd=2, grid_bwd=2)
    # ---- descriptors: copy_rows 0 / 1 / T - 1 / T, src_elem 0, a window ending on its store's last element, a store that is one window;
    #      two workgroups, either with windows of both dtypes
    P.append(_route("desc-edges", T, 6, grids=G2, stores=[(0, "u16", T, 0, ()), (1, "f32", T + 13, 0, ())],
                    windows=[(0, 0, T, 0), (1, 0, T, 13 * BINS), (1, T, 0, 0), (0, 1, T - 1, BINS), (1, T - 1, 1, (T + 12) * BINS), (0, T - 1, 1, 0)]))
    for dt in ("u16", "f32"):
        P.append(_route("dtype-%s-alone" % dt, T, 3, ntm=1, nfm=1, chosen={0: ([(5, 4)], [(3, 2)])},
                        stores=[(0, dt, T + 20, 0, ()), (1, dt, T + 20, 1, ())], windows=[(0, 0, T, 40), (1, 9, T - 9, 0), (0, 2, T - 2, 18 * BINS)]))
    P.append(_route("stores-0-1-62-63", T, 8, ntm=1, nfm=1, chosen={i: ([(4 + i, 3)], [(5 * i, 2)]) for i in range(8)}, grids=G2))
    # ---- mask counts and positions on the gather route
    T1 = 194
    P.append(_route("masks-1-0-T194", T1, 4, ntm=1, chosen={0: ([(T1 - 1, 1)], ()), 1: ([(30, 70)], ()), 2: ([(0, T1)], ()), 3: ([(190, 10)], ())}))
    P.append(_route("masks-8-0-T194", T1, 4, ntm=K_XMAX_MASKS, chosen={
        0: ([(0, 1), (T1 - 1, 1), (31, 2), (32, 32), (100, 10), (105, 15), (190, 10)], ()),
        1: ([(30, 70), (150, 10), (150, 10), (120, 1)], ()),
        2: ([(0, T1)], ()),
        3: ([(63, 2), (95, 2), (127, 34)], ())}))   # word boundaries 64, 96, and 128 .. 160 with a word in between
    P.append(_route("masks-0-1", T, 4, nfm=1, chosen={0: ((), [(31, 2)]), 1: ((), [(0, 40)]), 2: ((), [(38, 7)])}))
    P.append(_route("masks-0-8", T, 4, nfm=K_XMAX_MASKS, chosen={
        0: ((), [(0, 1), (39, 1), (3, 2), (31, 2), (10, 1), (20, 3)]),
        1: ((), [(2, 5), (28, 8), (38, 7)]),
        2: ((), [(32, 8)]),
        3: ((), [(0, 40)])}))
    P.append(_route("masks-4-4-T66", 66, 3, ntm=4, nfm=4, chosen={
        0: ([(10, 10), (31, 2), (40, 1), (60, 6)], [(5, 4), (31, 2), (36, 4), (0, 1)]),
        1: ([(33, 33)], [(0, 40)]),
        2: ([(0, 1)], [(39, 1)])}))
    T2 = T_BITMAP
    P.append(_route("T256-gather", T2, 2, ntm=2, chosen={0: ([(T2 - 32, 32)], ()), 1: ([(T2 - 1, 1), (200, 30)], ())}))
    P.append(_route("T257-materialised", T2 + 1, 2, ntm=2, chosen={0: ([(T2 - 32, 33)], ()), 1: ([(T2, 1), (200, 30)], ())}, route="materialised"))
    # ---- mask counts past the gather's limit: the assembly kernel writes the batch
    h = K_XMAX_MASKS // 2
    for ntm, nfm in ((h + 1, h), (K_MAX_MASKS, 0), (0, K_MAX_MASKS), (K_MAX_MASKS // 2, K_MAX_MASKS // 2)):
        chosen = {i: ([(2 * k + i, 1 + k % 2) for k in range(ntm)], [(39 - 3 * k - i, 1 + k % 2) for k in range(min(nfm, 12))]) for i in range(3)}
        P.append(_route("masks-%d-%d-materialised" % (ntm, nfm), T, 3, ntm=ntm, nfm=nfm, chosen=chosen, route="materialised"))
    # ---- a0 tiles of the stride-1 first block: 64 rows, one more, two tiles and a row; the strided first block in tail mode, over
    #      two tiles, and with (T - K1) % S != 0
    mk = {0: ([(3, 5)], [(6, 3)]), 1: ([(60, 9)], [(30, 4)]), 2: ([(0, 2)], [(0, 40)])}
    for T3 in (bts.TT + 2, bts.TT + 3, 2 * bts.TT + 3):
        P.append(_route("stride1-T%d" % T3, T3, 3, ntm=1, nfm=1, chosen=mk))
    for T3, tag in ((197, "tail"), (212, "two-tile"), (213, "remainder")):
        P.append(_route("strided-T%d-%s" % (T3, tag), T3, 3, ntm=1, nfm=1, chosen=mk, model="STRIDED"))
    # ---- windows per workgroup
    P.append(_route("wg-B2", T, 2, grids=G2))
    P.append(_route("wg-B5-uneven", T, 5, ntm=1, chosen={i: ([(3 * i, 2)], ()) for i in range(5)}, grids=G2))
    two = 2 * K_XMAX_SAMPLES
    each = {i: ([(2 * i + 1, 1 + i % 3), (40 - i, i % 2)], [(i, 1), (20 + i, 2 + i % 3)]) for i in range(two + 1)}
    P.append(_route("wg-B16-eight-each", T, two, ntm=2, nfm=2, chosen=each, grids=G2))
    P.append(_route("wg-B17-materialised", T, two + 1, ntm=2, nfm=2, chosen=each, grids=G2, route="materialised"))
    P.append(_route("wg-B17-fwd4-bwd2-materialised", T, two + 1, ntm=2, nfm=2, chosen=each, grids=dict(grid_fwd=4, grid_bwd=2), route="materialised"))
    # ---- the kernel forms that stage x, over two tiles and a row
    T4 = 2 * bts.TT + 3
    for tag, opts in (("fwd-x6", dict(conv1_x6_fwd=1)), ("bwd-plain", dict(conv1_x6=0)), ("bwdw-x6", dict(bwd_first_wide=1)), ("pointwise-bf16", dict(pw_bf16=True)),
                      ("storage-bf16", dict(st_bf16=True))):
        P.append(_route("form-%s" % tag, T4, 4, ntm=1, nfm=1, chosen=mk, options=opts, grids=G2))
    # ---- the graph engine's gathering stem
    for T5, route in ((K_GXROWS - 1, "gather"), (K_GXROWS, "gather"), (K_GXROWS + 1, "materialised")):
        P.append(_route("graph-T%d-%s" % (T5, route), T5, 3, ntm=2, nfm=2, chosen={0: ([(0, 1), (T5 - 1, 1)], [(31, 2), (0, 1)]), 1: ([(30, 70), (32, 32)], [(28, 8)]),
                                                                                    2: ([(T5 - 4, 10)], [(38, 7), (3, 2)])}, model="INC", route=route))
    P.append(_route("graph-wg-B16-eight-each", 60, two, ntm=2, nfm=2, chosen=each, model="INC", grids=dict(grid_graph=2)))
    P.append(_route("graph-wg-B17-materialised", 60, two + 1, ntm=2, nfm=2, chosen=each, model="INC", grids=dict(grid_graph=2), route="materialised"))
    # ---- the assembly kernel's parts: T * 10 float4 groups over 1..8 workgroups per window
    for T6 in (194, T_MIN):
        for n in SPLITS:
            P.append(_case("split%d-T%d" % (n, T6), "batch", T=T6, stores=std_stores(T6), windows=std_windows(T6, 3), ntm=2, nfm=2, split=n,
                           masks=fill_masks(3, 2, 2, {0: ([(T6 // 2, 3)], [(7, 2)]), 1: ([(0, 1), (T6 - 1, 1)], [(0, 1), (39, 1)]), 2: ([(T6 // 3, T6 // 3)], [(18, 4)])})))
    P.append(_case("split-refused", "split-refused", T=T, stores=std_stores(T), windows=std_windows(T, 2), items=[("split-refused",)]))
    # ---- values, on the materialised route: window 0 reads rows 0.. of the store from row 0 on, rows 2..3 lie under a time mask
    u = [(0, 0, 0), (0, 1, 1), (0, 2, 65535), (1, 5, 0), (2, 7, 65535), (4, 39, 0)]
    P.append(_case("values-u16", "batch", T=T, stores=[(0, "u16", T, 3, tuple(u)), (1, "f32", T, 3, ())], windows=[(0, 0, T, 0), (0, 5, T - 5, 0)], ntm=1, nfm=1,
                   masks=[[(2, 2), (38, 2)], [(7, 2), (38, 2)]], items=[("value", n) for n in VALUES[:3]],
                   specials=[(0, 0, 0, 0.0), (0, 0, 1, 0.0390625), (0, 0, 2, 65535 * 0.0390625), (0, 2, 7, 0.0), (1, 5, 2, 65535 * 0.0390625)]))
    nan, pinf, ninf = 0x7fc01234, _f32(np.inf), _f32(-np.inf)
    f = [(0, 0, _f32(-0.0)), (0, 1, 1), (0, 2, _f32(np.finfo(np.float32).max)), (1, 3, nan), (1, 4, pinf), (1, 5, ninf), (2, 3, nan), (2, 4, pinf), (2, 5, ninf),
         (4, 38, nan), (4, 39, pinf), (5, 39, ninf), (6, 0, 0xffc00001)]
    P.append(_case("values-f32", "batch", T=T, stores=[(0, "u16", 2 * T, 4, ()), (1, "f32", T, 4, tuple(f))], windows=[(1, 0, T, 0), (1, 3, T - 3, 0)], ntm=1, nfm=1,
                   masks=[[(2, 2), (38, 2)], [(5, 2), (38, 2)]], items=[("value", n) for n in VALUES[3:]],
                   specials=[(0, 0, 0, "bits", _f32(-0.0)), (0, 0, 1, "bits", 1), (0, 0, 2, "bits", _f32(np.finfo(np.float32).max)), (0, 1, 3, "bits", nan),
                             (0, 1, 4, "bits", pinf), (0, 1, 5, "bits", ninf), (0, 2, 3, "bits", 0), (0, 2, 4, "bits", 0), (0, 2, 5, "bits", 0),
                             (0, 4, 38, "bits", 0), (0, 4, 39, "bits", 0), (0, 5, 39, "bits", 0), (0, 6, 0, "bits", 0xffc00001), (1, 4, 3, "bits", nan)]))
    # ---- seventeen masks are refused and leave the engine as it was
    nine, eight = K_MAX_MASKS // 2 + 1, K_MAX_MASKS // 2
    P.append(_case("masks-%d-%d-refused" % (nine, eight), "refused", T=T, stores=std_stores(T), windows=std_windows(T, 3), ntm=2, nfm=2,
                   masks=fill_masks(3, 2, 2, {0: ([(4, 4)], [(9, 3)]), 2: ([(40, 9)], [(0, 2)])}), items=[("masks", "refused", nine, eight)]))
    # ---- labels and weights riding along in the descriptors' mailbox, and set behind it
    P.append(_route("targets-ride-along", T, 5, ntm=1, nfm=1, chosen={1: ([(9, 4)], [(11, 3)])}, items=[("targets",)], targets=True))
    # ---- whole window lists
    P.append(_case("window-lists", "windows", T=T, stores=std_stores(T), windows=std_windows(T, 8)[:7],
                   items=[("window-list", "evaluate", "n%batch"), ("window-list", "evaluate", "n<batch"), ("window-list", "bn_reestimate")]))
    # ---- streaming: frame_value of the five streaming kernels, and the descriptors mine_clip emits
    for name in ("float", "int8", "graph", "graph-int8", "calibrate"):
        P.append(_case("stream-%s" % name, "stream", form=name, items=[("stream", name)]))
    P.append(_case("stream-mine-padded-track", "mine", items=[("stream", "mine")]))
    # ---- stores past 2^31 elements and 2^32 bytes
    P.append(_case("large-stores", "large", T=T, items=[("large-store",)], gpu_only=True))
    assert len({c["id"] for c in P}) == len(P)
    return tuple(P)


def plan():
    """The sweep: a deterministic list of cases, each a dict (id, kind, model, T, stores, windows, ntm, nfm, masks, route, options,
    grids, split, items, gpu_only)."""
    return list(_plan())


def emulated_plan():
    """The cases the CPU suite runs on the emulated kernels: the plan minus the cases marked gpu_only."""
    return [c for c in plan() if not c["gpu_only"]]


def uncovered(cases=None):
    cov = set()
    for c in plan() if cases is None else cases:
        cov |= case_items(c)
    return [i for i in required() if i not in cov]


def describe(case):
    return "%s (%s %s T=%d B=%d masks (%d, %d) route %s options %s grids %s)" % (
        case["id"], case["kind"], case["model"], case["T"], len(case["windows"]), case["ntm"], case["nfm"], case["route"], case["options"], case["grids"])


# ------------------------------------------------------------------------------------------ running a case
def arrays(case):
    from microwakeword_amd import native
    win = np.array([(s, pad, copy, 0, src) for s, pad, copy, src in case["windows"]], native.WINDOW_DTYPE).reshape(-1)
    nm = case["ntm"] + case["nfm"]
    masks = np.array(case["masks"], np.int32).reshape(len(case["windows"]), nm, 2) if nm else None
    return win, masks


def targets_of(B, k=0):
    y = ((np.arange(B) + k) % 2).astype(np.float32)
    w = (0.5 + 0.25 * ((np.arange(B) + 2 * k) % 5)).astype(np.float32)
    return y, w


@functools.lru_cache(maxsize=None)
def _oracle(model, T, mode):
    import engine_checks as ec
    if model == "INC":
        return ec.perturbed_inception_oracle(T, ec.INC)
    return ec.perturbed_oracle(T, flags=_flags(model, mode))


def _flags(model, mode=0):
    import engine_checks as ec
    return dict(ec.DEF if model == "DEF" else ec.NOTEBOOK, **({1: dict(pw_bf16=True), 2: dict(st_bf16=True)}.get(mode, {})))


class Eng:
    """The engine of a case: the model with random weights, the case's options and grids, its stores uploaded."""

    def __init__(self, lib, case, stores, fused, max_batch=None):
        import engine_checks as ec
        B = max_batch or max(len(case["windows"]), 2)
        self.case, self.inc = case, case["model"] == "INC"
        om = _oracle(case["model"], case["T"], mode_of(case))
        if self.inc:
            self.lay, self.eng = ec.make_inception_engine(lib, case["T"], B, om, ec.INC)
        else:
            self.lay, self.eng = ec.make_engine(lib, case["T"], B, om, flags=dict(_flags(case["model"]), **case["options"]))
        try:
            for k, v in case["grids"].items():
                self.eng.set_option(k, v)
            self.eng.set_option("fused_input", fused)
            for sid, a in stores.items():
                self.eng.upload_store(sid, a)
        except BaseException:
            self.eng.close()
            raise

    def ready(self, B):
        import engine_checks as ec
        if self.inc:   # dropout off: every run of the case sees the same mask
            self.eng.set_dropout_mask(np.ones((B, ec.eng_dense_inputs(self.lay)), np.uint8))

    def a0(self, B):
        if self.inc or mode_of(self.case) == 2:
            return np.zeros(0, np.float32)
        k1, c1, _, _, s = FIRST[self.case["model"]]
        n = B * ((self.case["T"] - k1) // s + 1) * c1
        got = self.eng.debug_read("a0", B, n)
        assert got.size == n
        return got.copy()

    def close(self):
        self.eng.close()


def _assemble_count(names):
    return sum(n == "assemble" for n in names)


def _check_route(case, fused, names, what):
    want = 0 if (fused and case["route"] == "gather") else 1
    assert _assemble_count(names) == want, "%s %s fused_input %d: %d assemble launches, the case is declared %s: %s" % (
        case["id"], what, fused, _assemble_count(names), case["route"], " ".join(names))


def run_route(lib, case):
    """Comparisons 1 - 4 of the module docstring on one model-route case."""
    from microwakeword_amd import native
    assert case["route"] == expected_route(case), describe(case)
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    assert check_observability(case, stores, ref) > 0, describe(case)
    win, masks = arrays(case)
    B = win.size
    y, sw = targets_of(B)
    outs = []
    for fused in (0, 1):
        e = Eng(lib, case, stores, fused)
        eng = e.eng
        try:
            eng.set_option("profile", 1)
            eng.set_targets(y, sw)
            eng.assemble(win, masks, case["ntm"], case["nfm"])
            e.ready(B)
            eng.forward(B, training=False)
            _check_route(case, fused, [n for n, _ in eng.profile_read()], "evaluation forward")
            got = dict(eval_z=eng.read_outputs(B, want_loss=False)[1].copy())
            eng.assemble(win, masks, case["ntm"], case["nfm"])
            e.ready(B)
            eng.train_step(B, 1e-3, flags=native.STEP_NO_APPLY)
            names = [n for n, _ in eng.profile_read()]   # before any call that would materialise x
            _check_route(case, fused, names, "train step")
            if e.inc:
                gc = graph_case(case, bool(fused))
                assert gs.route_of_profile(names) == gs.case_route(gc), "%s fused_input %d: profiled route %s" % (case["id"], fused, " ".join(names))
                xg = sorted({k.split("<")[0] for k in gs.case_kernels(gc) if "_xg_kernel" in k})
                assert xg == (["gconv_wgrad_xg_kernel", "gconv_xg_kernel"] if fused and case["route"] == "gather" else []), (case["id"], fused, xg)
            p, z, loss = eng.read_outputs(B)
            got.update(a0=e.a0(B), grads=eng.get_grads().copy(), p=p.copy(), z=z.copy(), loss=np.float32(loss))
            x = eng.get_batch(B)
        finally:
            e.close()
        assert same_bits(x, ref), "%s fused_input %d: the batch read back differs from the reference in %d cells, first at %s" % (
            case["id"], fused, int((bits(x) != bits(ref)).sum()), np.argwhere(bits(x) != bits(ref))[:4].tolist())
        assert np.isfinite(got["grads"]).all() and np.isfinite(got["z"]).all() and np.any(got["grads"] != 0), case["id"]
        outs.append(got)
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), "%s: %s differs between the gathered and the materialised batch (%d of %d values)" % (
            describe(case), k, int((bits(outs[0][k]) != bits(outs[1][k])).sum()), np.asarray(outs[0][k]).size)


def run_targets(lib, case):
    """Labels and weights set before the batch (they ride in the descriptors' mailbox; assemble_kernel threads 64 and 128 move them
    when it runs) and after it, on both routes: loss, probabilities and gradient are bit-identical across the four."""
    from microwakeword_amd import native
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    check_observability(case, stores, ref)
    win, masks = arrays(case)
    B = win.size
    y0, w0 = targets_of(B, 0)
    y1, w1 = targets_of(B, 1)
    assert not np.array_equal(y0, y1) and not np.array_equal(w0, w1)
    outs = {}
    for fused in (0, 1):
        for order in ("before", "after"):
            e = Eng(lib, case, stores, fused)
            eng = e.eng
            try:
                eng.set_targets(y0, w0)   # an earlier batch's targets: the step must not see them
                eng.assemble(win, masks, case["ntm"], case["nfm"])
                eng.forward(B, training=False)
                if order == "before":
                    eng.set_targets(y1, w1)
                    eng.assemble(win, masks, case["ntm"], case["nfm"])
                else:
                    eng.assemble(win, masks, case["ntm"], case["nfm"])
                    eng.set_targets(y1, w1)
                eng.train_step(B, 1e-3, flags=native.STEP_NO_APPLY)
                p, z, loss = eng.read_outputs(B)
                outs[(fused, order)] = dict(grads=eng.get_grads().copy(), p=p.copy(), loss=np.float32(loss))
                assert same_bits(eng.get_batch(B), ref), (case["id"], fused, order)
            finally:
                e.close()
    # ... and they are the targets' own: another label set gives another loss
    e = Eng(lib, case, stores, 1)
    try:
        e.eng.set_targets(y0, w0)
        e.eng.assemble(win, masks, case["ntm"], case["nfm"])
        e.eng.train_step(B, 1e-3, flags=native.STEP_NO_APPLY)
        assert np.float32(e.eng.read_outputs(B)[2]) != outs[(1, "before")]["loss"], case["id"]
    finally:
        e.close()
    first = outs[(0, "before")]
    for key, got in outs.items():
        for k in first:
            assert same_bits(first[k], got[k]), "%s: %s differs at fused_input %d, targets %s the batch" % (case["id"], k, key[0], key[1])


def run_batch(lib, case):
    """The materialised batch against the reference ("fused_input" 0, the case's "assemble_split")."""
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    check_observability(case, stores, ref)
    for s in case.get("specials", ()):
        i, t, f = s[:3]
        want = s[4] if s[3] == "bits" else int(np.array([s[3]], np.float32).view(np.uint32)[0])
        assert int(bits(ref)[i, t, f]) == want, "%s: the reference holds %#x at %s, the plan says %#x" % (case["id"], int(bits(ref)[i, t, f]), (i, t, f), want)
    win, masks = arrays(case)
    B = win.size
    e = Eng(lib, case, stores, 0)
    try:
        if case["split"] is not None:
            e.eng.set_option("assemble_split", case["split"])
        e.eng.set_option("profile", 1)
        e.eng.assemble(win, masks, case["ntm"], case["nfm"])
        x = e.eng.get_batch(B)
        assert _assemble_count([n for n, _ in e.eng.profile_read()]) == 1, case["id"]
    finally:
        e.close()
    diff = bits(x) != bits(ref)
    assert not diff.any(), "%s: %d cells differ from the reference, first at %s" % (describe(case), int(diff.sum()), np.argwhere(diff)[:4].tolist())


def run_refused(lib, case):
    """One mask more than kMaxMasks is refused with the library's error and leaves the engine as it was: the next valid batch
    gives the bytes a fresh engine gives."""
    import pytest
    from microwakeword_amd import native
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    check_observability(case, stores, ref)
    win, masks = arrays(case)
    B = win.size
    ntm, nfm = K_MAX_MASKS // 2 + 1, K_MAX_MASKS // 2
    bad = np.zeros((B, ntm + nfm, 2), np.int32)
    bad[:, :, 0], bad[:, :, 1] = 3, 2
    got = []
    for refuse in (True, False):
        e = Eng(lib, case, stores, 1)
        try:
            e.eng.assemble(win[::-1].copy(), masks[::-1].copy(), case["ntm"], case["nfm"])
            if refuse:
                with pytest.raises(native.NativeError, match="too many masks"):
                    e.eng.assemble(win, bad, ntm, nfm)
                assert same_bits(e.eng.get_batch(B), ref[::-1]), case["id"] + ": the refused call changed the batch held"
            e.eng.assemble(win, masks, case["ntm"], case["nfm"])
            got.append(e.eng.get_batch(B))
        finally:
            e.close()
    assert same_bits(got[0], got[1]) and same_bits(got[0], ref), case["id"]


def run_split_refused(lib, case):
    import pytest
    from microwakeword_amd import native
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    win, masks = arrays(case)
    e = Eng(lib, case, stores, 0)
    try:
        for v in (SPLIT_RANGE[0] - 1, SPLIT_RANGE[1] + 1):
            with pytest.raises(native.NativeError, match="assemble_split out of range"):
                e.eng.set_option("assemble_split", v)
        e.eng.assemble(win, masks, 0, 0)
        assert same_bits(e.eng.get_batch(win.size), ref), case["id"]
    finally:
        e.close()


def _metric_bytes(eng):
    import ctypes
    m = eng.metrics_raw()
    return ctypes.string_at(ctypes.addressof(m), ctypes.sizeof(m))


def run_windows(lib, case):
    """mww_evaluate_windows and mww_bn_reestimate_windows over a list that mixes dtypes, stores 0 and 63 and pad_rows 0 and above,
    against the same windows run batch by batch through assemble + forward(update_metrics) / bn_reestimate_batch: logits of the
    last batch, metric counters and re-estimated statistics are bit-identical.  (mww_bn_reestimate_windows takes whole batches
    only: its list is the first six windows.)"""
    stores = build_stores(case)
    ref = reference_batch(case, stores)
    check_observability(case, stores, ref)
    win, _ = arrays(case)
    n = win.size
    assert {int(s) for s in win["store"]} >= {0, MAX_STORES - 1} and (win["pad_rows"] == 0).any() and (win["pad_rows"] > 0).any()
    labels = targets_of(n)[0]
    for batch, count in ((3, n), (3, 2)):   # n = 7 is no multiple of the batch; n = 2 is below it
        assert (count % batch != 0) if count > batch else count < batch
        got = []
        for whole in (True, False):
            e = Eng(lib, case, stores, 1, max_batch=batch)
            try:
                if whole:
                    e.eng.evaluate_windows(win[:count], labels[:count], batch)
                else:
                    for s in range(0, count, batch):
                        b = min(batch, count - s)
                        e.eng.set_targets(labels[s:s + b], np.ones(b, np.float32))
                        e.eng.assemble(win[s:s + b], None, 0, 0)
                        e.eng.forward(b, training=False, update_metrics=True)
                last = count - (count - 1) // batch * batch
                got.append((_metric_bytes(e.eng), e.eng.read_outputs(last, want_loss=False)[1].copy(), e.eng.get_batch(last)))
            finally:
                e.close()
        assert got[0][0] == got[1][0], "%s: metric counters of %d windows in batches of %d differ" % (case["id"], count, batch)
        assert same_bits(got[0][1], got[1][1]) and same_bits(got[0][2], got[1][2]), case["id"]
        assert same_bits(got[0][2], ref[count - got[0][2].shape[0]:count]), case["id"]
    got = []
    for whole in (True, False):
        e = Eng(lib, case, stores, 1, max_batch=3)
        try:
            e.eng.set_weight_ema(0.9, 1)
            e.eng.set_targets(labels[:3], np.ones(3, np.float32))
            e.eng.assemble(win[:3], None, 0, 0)
            e.eng.train_step(3, 1e-3)   # the average takes an update
            if whole:
                e.eng.bn_reestimate_windows(win[:6], 3)
            else:
                e.eng.bn_reestimate_begin()
                for s in (0, 3):
                    e.eng.assemble(win[s:s + 3], None, 0, 0)
                    e.eng.bn_reestimate_batch(3)
                e.eng.bn_reestimate_commit()
            state, valid = e.eng.get_ema_bn_state()
            assert valid
            got.append(state.copy())
        finally:
            e.close()
    assert same_bits(got[0], got[1]), "%s: re-estimated statistics differ in %d values" % (case["id"], int((bits(got[0]) != bits(got[1])).sum()))
    assert np.isfinite(got[0]).all() and np.any(got[0] != 0)


# ---- streaming
STREAM_CASE = "tiny"             # tests/stream_sweep.py: the model of the float / int8 / calibration cases
STREAM_GRAPH_CASE = None         # tests/stream_graph_sweep.py: the first case of its plan


def stream_tracks(T):
    """Four tracks with pad_rows above 0, both dtypes in one call, stores 0, 1 and 63: (store specs, windows)."""
    stores = std_stores(3 * T)
    return stores, [(MAX_STORES - 1, 5, 2 * T, 3 * BINS), (1, 0, T + 3, 0), (0, T // 2, T, (2 * T + 20) * BINS), (MAX_STORES - 2, 3, 1, 7 * BINS)]


def track_frames(stores, windows):
    out = []
    for sid, pad, copy, src in windows:
        rows = stores[sid].reshape(-1, BINS)[src // BINS:src // BINS + copy]
        rows = rows.astype(np.float32) * np.float32(0.0390625) if rows.dtype == np.uint16 else rows
        out.append(np.concatenate([np.zeros((pad, BINS), np.float32), rows], 0))
    return out


def _stream_built(form):
    if form.startswith("graph"):
        import stream_graph_sweep as sg
        return sg, sg.built(sg.case_ids()[0])
    import stream_sweep as ss
    return ss, ss.built(ss.case_ids()[0])


def run_stream(lib, case):
    """mww_stream_run over tracks of the resident stores against mww_stream_run_host on the same frames materialised by NumPy:
    probabilities, logits and the final state (the calibration form: the recorded ranges) are bit-identical."""
    from microwakeword_amd import native, streaming
    import streaming_checks as sc
    form = case["form"]
    graph = form.startswith("graph")
    mod, b = _stream_built(form)
    s = 1 if graph else b.s
    T = int(b.desc["frames"])
    specs, windows = stream_tracks(max(T, 8) * s)
    windows = [(sid, pad - pad % s, copy - copy % s if copy >= s else s, src) for sid, pad, copy, src in windows]   # whole strides: no row is dropped
    stores = {spec[0]: build_store(spec) for spec in specs}
    frames = track_frames(stores, windows)
    win = np.array([(sid, pad, copy, 0, src) for sid, pad, copy, src in windows], native.WINDOW_DTYPE)
    assert (win["pad_rows"] > 0).any() and len({stores[int(i)].dtype for i in win["store"]}) == 2 and MAX_STORES - 1 in win["store"]
    # a wrong pad, source row, dtype or store would feed other frames
    obs = dict(id=case["id"], T=0, ntm=0, nfm=0, masks=[[] for _ in windows])
    for i, w in enumerate(windows):
        c1 = dict(obs, T=w[1] + w[2], windows=[w], masks=[[]])
        assert check_observability(c1, stores, reference_batch(c1, stores)) > 0
    model = sc.context_model(lib)
    for sid, a in stores.items():
        model.engine.upload_store(sid, a)

    def fresh():
        if form in ("float", "graph"):
            st = (native.GraphStream if graph else native.Stream)(model.engine, b.desc)
            st.set_weights(b.flat)
            return st
        if form == "calibrate":
            st = native.Stream(model.engine, b.desc, int8=True)
            st.set_weights(b.flat)
            return st
        return streaming.QuantizedStreamingModel(b.qm, s, "stream", context=model).native

    q8 = form.endswith("int8")
    got = []
    for resident in (True, False):
        st = fresh()
        try:
            if form == "calibrate":
                if resident:
                    off, ranges = st.calibrate(win)
                    assert list(np.diff(off)) == [len(f) // s for f in frames], (case["id"], off)
                else:
                    ranges = st.calibrate_host(np.concatenate(frames, 0))
                got.append((st.read().copy(), ranges.copy(), bits(st.get_state()).copy()))
                continue
            if resident:
                off = st.run(win)
                assert list(np.diff(off)) == [len(f) // s for f in frames], (case["id"], off)
            else:
                assert st.run_host(np.concatenate(frames, 0)) == sum(len(f) // s for f in frames)
            p, z = st.read(want_logits=True)
            state = st.get_state_q8().view(np.uint8).copy() if q8 else bits(st.get_state()).copy()
            got.append((p.copy(), z.copy(), state) + ((st.read_q8().copy(),) if q8 else ()))
        finally:
            st.close()
    assert got[0][0].size == sum(len(f) // s for f in frames) and got[0][0].size > 0 and np.isfinite(got[0][0]).all(), case["id"]
    assert len(np.unique(got[0][0])) > 1, case["id"] + ": the outputs do not depend on the frames"
    for k, (a, c) in enumerate(zip(got[0], got[1])):
        assert a.shape == c.shape and np.array_equal(a.view(np.uint8), c.view(np.uint8)), "%s: output %d of the resident tracks differs from the host frames (%d values)" % (
            case["id"], k, int((a.view(np.uint8) != c.view(np.uint8)).sum()))


def run_mine(lib, case):
    """One detection in a padded track: the clip mine_clip emits, assembled, equals the NumPy slice of the track's rows
    [e - frames - before, e + after) that exist in the store."""
    from microwakeword_amd import native
    import stream_sweep as ss
    import streaming_checks as sc
    model = sc.context_model(lib)
    T = model.engine.frames
    desc = dict(ss.desc_of(4, 3, 1, [(1, (3,), 8)], 2), mode="stream")
    frames = int(desc["frames"])
    specs = std_stores(100)
    stores = {spec[0]: build_store(spec) for spec in specs}
    for sid, a in stores.items():
        model.engine.upload_store(sid, a)
    pad, copy, src = 9, 80, 11 * BINS
    tracks = [(0, 0, 30, 0), (MAX_STORES - 1, pad, copy, src), (1, 2, 40, 5 * BINS)]
    win = np.array([(sid, p, c, 0, s0) for sid, p, c, s0 in tracks], native.WINDOW_DTYPE)
    lengths = [p + c for _, p, c, _ in tracks]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    window, before, after = 5, 12, 20
    for at in (4, 40):   # the moving-average index of the detection: a clip the pad clips, and one inside the track
        probs = np.zeros(int(off[-1]), np.float32)
        probs[off[1] + at:off[1] + at + window] = 1.0
        st = native.Stream(model.engine, desc)
        try:
            st.set_probs(probs)
            clips, events, total, counts = st.mine(win, off, 0.9, window, 0, before, after)
        finally:
            st.close()
        assert total == 1 and clips.size == 1 and list(counts) == [0, 1, 0] and int(events["index"][0]) == at, (case["id"], at, clips, events)
        end = at + window   # the track row behind the last frame of the window that fired (stride 1, stream mode)
        track = track_frames(stores, [tracks[1]])[0]
        lo, hi = max(end - frames - before, pad), min(end + after, pad + copy)
        want = track[lo:hi]
        c = clips[0]
        assert int(c["store"]) == MAX_STORES - 1 and int(c["pad_rows"]) == 0 and int(c["copy_rows"]) == hi - lo, (case["id"], at, c)
        assert (lo == pad) == (at == 4), case["id"]
        rows = int(c["copy_rows"])
        fit = np.array([(int(c["store"]), T - rows, rows, 0, int(c["src_elem"]))], native.WINDOW_DTYPE)
        model.engine.assemble(fit, None, 0, 0)
        x = model.engine.get_batch(1)[0]
        assert same_bits(x[T - rows:], want) and not x[:T - rows].any(), "%s: the clip at %d reads other rows" % (case["id"], at)
        assert not same_bits(track[lo + 1:hi + 1], want) and not same_bits(track[lo - 1:hi - 1], want)


# ---- large stores
def large_windows(dtype, T):
    """(rows of the store, [(first row, tag)]) of the windows of a large store: they straddle byte offsets 2^31 and 2^32, in the
    uint16 store element index 2^31, and end on the store's last row."""
    size = 2 if dtype == "u16" else 4
    n = (2 ** 31 if dtype == "u16" else 2 ** 30) + BINS * 512
    rows = -(-n // BINS)   # mww_upload_store takes whole rows: the first multiple of 40 elements at or above 2^31 (2^30) + 40 * 512
    assert 0 <= rows * BINS - n < BINS
    at = []
    for byte in (2 ** 31, 2 ** 32):
        r = byte // (BINS * size)   # the row that holds the byte (2^31 and 2^32 are no multiples of a row)
        at.append((r - T // 2, "byte-2^%d" % (31 if byte == 2 ** 31 else 32)))
    if dtype == "u16":
        assert (2 ** 31 // BINS - T // 2, "byte-2^32") == at[1]   # element 2^31 of the uint16 store is its byte 2^32
    at.append((rows - T, "last-row"))
    at.append((0, "first-row"))
    return rows, at


def run_large(lib, case, dtypes=("u16", "f32")):
    """Stores past 2^31 elements / 2^32 bytes through every route of one engine each: the materialised batch, the block gather
    forward and backward, whole window lists, one streaming track and one mined clip; the graph stem in an engine of its own.
    Every window holds its own random pattern in a store that is zero elsewhere: an index that wrapped modulo 2^32 reads zeros or
    another window's pattern."""
    from microwakeword_amd import native
    import engine_checks as ec
    import stream_sweep as ss
    T = case["T"]
    for dtype in dtypes:
        rows, at = large_windows(dtype, T)
        big = np.zeros(rows * BINS, np.uint16 if dtype == "u16" else np.float32)
        eng = geng = st = None
        try:
            view = big.reshape(-1, BINS)
            for k, (r, _) in enumerate(at):
                view[r:r + T] = build_store((k, dtype, T, 7, ())).reshape(T, BINS)
            sid = MAX_STORES - 1
            stores = {sid: big}
            windows = [(sid, 0, T, r * BINS) for r, _ in at] + [(sid, 3, T - 3, at[0][0] * BINS), (sid, T - 1, 1, (rows - 1) * BINS)]
            c = _case(case["id"] + "-" + dtype, "route", T=T, windows=windows, ntm=1, nfm=1, route="gather",
                      masks=fill_masks(len(windows), 1, 1, {0: ([(T // 2 - 1, 2)], [(8, 2)])}))
            ref = np.stack([reference(big, w, *window_masks(c, i), T) for i, w in enumerate(windows)])
            assert len({ref[i].tobytes() for i in range(len(windows))}) == len(windows) and all(r.any() for r in ref)
            for i in range(len(windows)):   # src_elem +-40 shows; so would the low 32 bits alone
                for name, s2, w2, tm, fm in neighbours(c, stores, i):
                    if name.startswith(("src_elem", "pad_rows")):
                        assert not same_bits(reference(big, w2, tm, fm, T), ref[i]), (c["id"], i, name)
            assert any(w[3] * big.itemsize >= 2 ** 32 for w in windows) and (dtype != "u16" or any(w[3] >= 2 ** 31 for w in windows))
            win, masks = arrays(c)
            B = win.size
            y, sw = targets_of(B)
            om = _oracle("DEF", T, 0)
            outs = []
            lay, eng = ec.make_engine(lib, T, B, om)
            eng.upload_store(sid, big)
            state = eng.get_bn_state()
            for fused in (0, 1):
                eng.set_bn_state(state)   # (the first pass's train step moved the moving statistics)
                eng.set_option("fused_input", fused)
                eng.set_option("profile", 1)
                eng.set_targets(y, sw)
                eng.assemble(win, masks, 1, 1)
                eng.forward(B, training=False)
                z = eng.read_outputs(B, want_loss=False)[1].copy()
                eng.assemble(win, masks, 1, 1)
                eng.train_step(B, 1e-3, flags=native.STEP_NO_APPLY)
                names = [n for n, _ in eng.profile_read()]
                assert _assemble_count(names) == 2 * (1 - fused), (c["id"], fused, names)
                outs.append(dict(z=z, grads=eng.get_grads().copy(), p=eng.read_outputs(B)[0].copy()))
                x = eng.get_batch(B)
                assert same_bits(x, ref), "%s fused_input %d: %d cells of the batch differ" % (c["id"], fused, int((bits(x) != bits(ref)).sum()))
                eng.set_option("profile", 0)
            for k in outs[0]:
                assert same_bits(outs[0][k], outs[1][k]), "%s: %s differs between the gathered and the materialised batch" % (c["id"], k)
            # whole window lists against batch by batch
            eng.metrics_reset()
            eng.evaluate_windows(win, y, 3)
            whole = _metric_bytes(eng)
            eng.metrics_reset()
            for s in range(0, B, 3):
                b = min(3, B - s)
                eng.set_targets(y[s:s + b], np.ones(b, np.float32))
                eng.assemble(win[s:s + b], None, 0, 0)
                eng.forward(b, training=False, update_metrics=True)
            assert whole == _metric_bytes(eng), c["id"]
            # one streaming track across byte 2^32 and one mined clip whose src_elem exceeds 2^32
            desc = dict(ss.desc_of(4, 3, 1, [(1, (3,), 8)], 2), mode="stream")
            frames = int(desc["frames"])
            r32 = at[1][0]
            track = (sid, 2, T, r32 * BINS)
            tf = track_frames(stores, [track])[0]
            st = native.Stream(eng, desc)
            st.set_weights(np.random.default_rng(SEED).normal(0, 0.3, st.n_weights).astype(np.float32))
            off = st.run(np.array([(sid, 2, T, 0, r32 * BINS)], native.WINDOW_DTYPE))
            p0 = st.read().copy()
            st.reset()
            assert st.run_host(tf) == int(off[-1]) == T + 2
            assert same_bits(p0, st.read()) and len(np.unique(p0)) > 1, c["id"] + ": the streamed track differs from its frames"
            hi_row = rows - T   # the store's last window
            trk = np.array([(sid, 1, T, 0, hi_row * BINS)], native.WINDOW_DTYPE)
            probs = np.zeros(T + 1, np.float32)
            probs[20:25] = 1.0
            st.set_probs(probs)
            clips, events, total, _ = st.mine(trk, np.array([0, T + 1], np.int64), 0.9, 5, 0, 0, 0)
            assert total == 1 and clips.size == 1, (c["id"], clips)
            end = 25
            lo = end - frames - 1
            assert int(clips[0]["src_elem"]) == (hi_row + lo) * BINS and int(clips[0]["copy_rows"]) == frames, (c["id"], clips)
            assert int(clips[0]["src_elem"]) * big.itemsize > 2 ** 32 and (dtype != "u16" or int(clips[0]["src_elem"]) > 2 ** 31)
            fit = np.array([(sid, T - frames, frames, 0, int(clips[0]["src_elem"]))], native.WINDOW_DTYPE)
            eng.assemble(fit, None, 0, 0)
            want = track_frames(stores, [(sid, 0, frames, (hi_row + lo) * BINS)])[0]
            assert same_bits(eng.get_batch(1)[0][T - frames:], want) and want.any(), c["id"]
            st.close()
            st = None
            eng.close()
            eng = None
            # the graph stem
            gom = _oracle("INC", T, 0)
            outs = []
            glay, geng = ec.make_inception_engine(lib, T, B, gom, ec.INC)
            geng.upload_store(sid, big)
            state = geng.get_bn_state()
            for fused in (0, 1):
                geng.set_bn_state(state)
                geng.set_option("fused_input", fused)
                geng.set_option("profile", 1)
                geng.set_targets(y, sw)
                geng.assemble(win, masks, 1, 1)
                geng.set_dropout_mask(np.ones((B, ec.eng_dense_inputs(glay)), np.uint8))
                geng.train_step(B, 1e-3, flags=native.STEP_NO_APPLY)
                names = [n for n, _ in geng.profile_read()]
                assert _assemble_count(names) == 1 - fused, (c["id"], fused, names)
                outs.append(dict(grads=geng.get_grads().copy(), p=geng.read_outputs(B)[0].copy()))
                assert same_bits(geng.get_batch(B), ref), c["id"]
                geng.set_option("profile", 0)
            for k in outs[0]:
                assert same_bits(outs[0][k], outs[1][k]), "%s: graph stem: %s differs between the gathered and the materialised batch" % (c["id"], k)
        finally:
            for h in (st, eng, geng):
                if h is not None:
                    h.close()
            del big


RUNNERS = {"route": run_route, "batch": run_batch, "refused": run_refused, "split-refused": run_split_refused, "windows": run_windows,
           "stream": run_stream, "mine": run_mine, "large": run_large}


def run_case(lib, case):
    """Run one case of plan() on ``lib``; every engine and stream it creates is closed however it ends."""
    if case.get("targets"):
        return run_targets(lib, case)
    return RUNNERS[case["kind"]](lib, case)
