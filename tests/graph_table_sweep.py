"""A covering sweep of the generic conv/BN graph training kernels (csrc/kernels_graph.hip.h, graph_launch.hip.h, tu_graph.hip,
graph_engine.hip), shared by the GPU sweep (tests/test_graph_table_sweep_gpu.py), its CPU-side checks
(tests/test_graph_table_sweep_emulated.py) and tools/table_sweep_kernels.py --graph.  The manner of tests/block_table_sweep.py:

- ``tables()`` reads the instantiation tables from graph_launch.hip.h itself ("the one place that lists instantiations"; this
  engine has no host-side probe) with a small X-macro parser - the non-MWW_SLIM branch of every #ifdef;
- ``build_graph()`` restates plan_ops of graph_engine.hip over the op list of a layout (microwakeword_amd/layout.py): twins,
  planar tensors, the statistics hand-over, the automatic frame-chunk setting; ``instantiation(role, op, ctx)`` restates the
  dispatch of graph_engine.hip and tu_graph.hip - static shape, frame chunks, fused pair or weight-gradient + data-gradient
  launches - and returns the demangled template a launch runs (``gconv_bwd_chunk_kernel<48, 32>``, ``gconv_kernel<60, 1>``,
  ``gconv_kernel<24, 0, GSh1>`` for a static shape).  Every fallback of the C++ is silent, so ``case_route()`` - the launch
  names "profile" 1 records - is compared with the engine per case, and a kernel trace of the GPU sweep with ``inventory()``;
- ``plan()`` is a deterministic, seeded list of small train-step cases, each an Inception or MixedNet *flag set* (the
  vocabulary of oracle/model_oracle.py and of the product) with B, T, grid, engine options and fuse_heads, that covers
  ``required()``: every instantiation of the inventory and the axis items below.

Axis items (the terms of required() next to the instantiation names):
  ("auto" | "grid2", inst)    a fused-pair instantiation, or a weight-gradient / data-gradient instantiation of the two-launch
                              route, under per-launch grids with the role split, and under "grid_graph" 2 with B = 5 (a
                              workgroup loops over 3 and 2 windows; the two roles of a fused launch get one workgroup each)
  ("dgrad-share", 10|30|90)   a fused pair under per-launch grids with that "graph_dgrad_share"
  ("B<grid",)                 fewer windows than the fixed grid
  ("S", inst, 2|3|4)          a frame-chunk instantiation under "graph_frame_chunks" 2, 3 and 4 (every CH instantiation under
                              every S)
  ("short-chunk", S)          an op whose frames S does not divide
  ("tout", 31|32|33)          the threshold of chunking (31 on the whole-window kernels)
  ("auto-chunks", S)          the automatic setting's 40 KB rule arriving at S > 1
  ("kparts", 4|2|1, "fused" | "split")   gwg_kparts over k * cin <= 16, 17..32, > 32
  ("dw-taps", k), ("dw-ch", c), ("dw-bias", bool), ("dw-mix1",)   depthwise ops
  ("ssn", groups, "handover" | "finalize"), ("twin-finalize2",)
  ("static", planar, fuse_heads, T)       the default Inception flags on both sides of kGTmax
  ("gather", 200 | 201 | "overflow")      the gathering stem (kGXRows, kXMaxSamples)
  ("head", "att" | "avg" | "max" | "att+pool"), ("residual-two-adders",)

Conditioning of the comparison (the constants of block_table_sweep.py for fp32): at least MIN_FINAL_FRAMES frames reach the
dense layer and at least MIN_BN_ROWS rows every BatchNorm, so that the comparison, not the kernel, stays well-posed; no MixedNet
case may hold a unit within float32 rounding of a ReLU zero or an attention tie (engine_checks.graph_mixednet_near_zero): the
planner redraws the case's seed until the count is 0, and the GPU test runs check_graph_mixednet with strict=True."""
import functools
import os
import random
import re

from oracle import model_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_H = os.path.join(ROOT, "microwakeword_amd", "csrc", "graph_launch.hip.h")

# constants of the kernels and the engine (common.hip.h, kernels_fwd.hip.h, kernels_graph.hip.h, graph_engine.hip)
K_THREADS = 256
FEATURE_BINS = 40
K_GTMAX = 208          # kGTmax: rows of a static shape's window
K_GXROWS = 200         # kGXRows: frames of a gathered window
K_XMAX_SAMPLES = 8     # kXMaxSamples: windows per workgroup of a gathering launch
K_GFOLDC = 64          # kGFoldC
K_MAX_DYN_LDS = 144 * 1024

MIN_FINAL_FRAMES = 8
MIN_BN_ROWS = 32

_ARITY = dict(MWW_G_WIDTHS=1, MWW_G_SHAPES=9, MWW_G_SHAPE_FWD=2, MWW_G_SHAPE_FWD2=2, MWW_G_SHAPE_WG=2, MWW_G_SHAPE_XG=2,
              MWW_G_SHAPE_BWD=3, MWW_G_SHAPE_BWD2=2, MWW_G_BWD_PAIRS=2, MWW_G_TWIN_WIDTHS=1)

# The fused pairs and twin widths of graph_launch.hip.h when this plan was last reviewed.  The planner reads the header, so a
# pair or a twin width deleted there would quietly be re-planned as two launches / two single ops - the very fallback this sweep
# exists to catch.  The coverage test holds the header to this list in both directions: change both together.
PINNED_PAIRS = ((30, 24), (10, 10), (10, 30), (30, 10), (48, 10), (16, 16), (16, 48), (24, 16), (16, 24), (36, 24), (12, 36), (48, 32),
                (48, 48), (64, 32), (64, 64))
PINNED_TWINS = (8, 10, 12, 16, 20, 24, 32)


def pinned_instantiations():
    out = set()
    for a, b in PINNED_PAIRS:
        out |= {"gconv_bwd_kernel<%d, %d>" % (a, b), "gconv_bwd_chunk_kernel<%d, %d>" % (a, b)}
    for n in PINNED_TWINS:
        out |= {"gconv_fwd2_kernel<%d>" % n, "gconv_bwd2_kernel<%d, %d>" % (n, n)}
    return out


# Table entries and axis items no Inception or MixedNet flag set reaches: {item: why}.  uncovered() must equal this set.
UNREACHABLE = {
    "gconv_fwd2_kernel<24>": "twins are Inception's second-level convolutions of width cnn2_filters1 = 24; the block's 1x1 over the concatenation then reads 72 channels, not an instantiated width (plan_ops refuses the model)",
    "gconv_bwd2_kernel<24, 24>": "as gconv_fwd2_kernel<24>",
    "gconv_fwd2_kernel<32>": "as width 24: the concatenation would hold 96 channels",
    "gconv_bwd2_kernel<32, 32>": "as gconv_fwd2_kernel<32>",
    "gconv_bwd_kernel<10, 10, GSh3>": "shape 3 (a 10-channel slice of the fused, row-stored heads) belongs to a block's two second-level convolutions, which always form a twin; they run singly only under sync-BN data parallelism, or under \"profile_split\", which also splits the backward launch; it runs in the INC cases of tests/exchange_checks.py (sync-BN ranks replayed on one device), which no plan of this sweep can express",
    "gconv_bwd_kernel<16, 16, GSh7>": "as gconv_bwd_kernel<10, 10, GSh3>, for the 16-channel block (the same cases of tests/exchange_checks.py)",
    ("dw-taps", 1): "a MixedNet block of kernel size 1 has no depthwise op (mixednet.py); a 1-tap group of a MixConv is covered as (\"dw-mix1\",)",
    ("dw-bias", False): "every depthwise op of a MixedNet has a bias (layout.GraphMixedNetLayout: norm \"bias\")",
}


# ------------------------------------------------------------------------------------------ tables
def _parse_tables(text):
    lines, stack = [], []   # stack of (macro, in_else) of open #if blocks
    for raw in text.split("\n"):
        s = raw.strip()
        if s.startswith(("#ifdef", "#ifndef", "#if ")):
            stack.append([s.split()[1] if len(s.split()) > 1 else "", s.startswith("#ifndef")])
            continue
        if s.startswith("#else"):
            stack[-1][1] = not stack[-1][1]
            continue
        if s.startswith("#endif"):
            stack.pop()
            continue
        # keep a line unless it sits in the MWW_SLIM branch (#ifdef MWW_SLIM ... before its #else)
        if any(m == "MWW_SLIM" and not taken for m, taken in stack):
            continue
        lines.append(raw)
    joined = re.sub(r"\\\s*\n", " ", "\n".join(lines))
    out = {}
    for m in re.finditer(r"^#define (MWW_G_\w+)\(X\)(.*)$", joined, re.M):
        name, body = m.group(1), m.group(2).split("//")[0]
        if name not in _ARITY:
            continue
        entries = re.findall(r"X\(([^()]*)\)", body)
        if re.sub(r"X\([^()]*\)", "", body).strip():
            raise ValueError("%s: cannot parse %r" % (name, body.strip()))
        rows = []
        for e in entries:
            try:
                row = tuple(int(v) for v in e.split(","))
            except ValueError:
                raise ValueError("%s: entry X(%s) is not a list of integers" % (name, e)) from None
            if len(row) != _ARITY[name]:
                raise ValueError("%s: entry X(%s) has %d fields, not %d" % (name, e, len(row), _ARITY[name]))
            rows.append(row[0] if _ARITY[name] == 1 else row)
        if name in out:
            raise ValueError("%s is defined twice outside MWW_SLIM" % name)
        out[name] = tuple(rows)
    missing = sorted(set(_ARITY) - set(out))
    if missing:
        raise ValueError("graph_launch.hip.h: no definition of %s" % ", ".join(missing))
    if not out["MWW_G_WIDTHS"] or not out["MWW_G_BWD_PAIRS"]:
        raise ValueError("graph_launch.hip.h: empty width or pair table")
    return out


@functools.lru_cache(maxsize=None)
def _tables(path):
    with open(path) as fh:
        t = _parse_tables(fh.read())
    return dict(widths=t["MWW_G_WIDTHS"], shapes={r[0]: r[1:] for r in t["MWW_G_SHAPES"]}, fwd=frozenset(t["MWW_G_SHAPE_FWD"]),
                fwd2=frozenset(t["MWW_G_SHAPE_FWD2"]), wg=frozenset(t["MWW_G_SHAPE_WG"]), xg=frozenset(t["MWW_G_SHAPE_XG"]),
                bwd=frozenset(t["MWW_G_SHAPE_BWD"]), bwd2=frozenset(t["MWW_G_SHAPE_BWD2"]), pairs=frozenset(t["MWW_G_BWD_PAIRS"]),
                twins=frozenset(t["MWW_G_TWIN_WIDTHS"]))


def tables(path=LAUNCH_H):
    """The instantiation tables of graph_launch.hip.h (non-MWW_SLIM branch): widths, shapes {id: (K, sources, C0, LD0, C1, LD1, C2,
    LD2)}, fwd / fwd2 / wg / xg {(id, filters)}, bwd {(id, filters, input channels)}, bwd2 {(id, width)}, pairs {(filters, input
    channels)}, twins {width}.  ValueError if a macro is missing or an entry does not parse."""
    return _tables(path)


# ------------------------------------------------------------------------------------------ plan_ops, restated
def _up4(v):
    return (v + 3) & ~3


def _up16(v):
    return (v + 15) // 16 * 16


def gwg_kparts(tasks):
    return 1 if tasks > 32 else (2 if tasks > 16 else 4)


def _lds_body(tiles, pairs):
    return (max(tiles, 2 * K_THREADS) + pairs * 2 * K_THREADS + 4) * 4


def _lds_fwd(o, rin, rout):
    return _lds_body(o["k"] * _up4(o["cin"]) * _up16(o["cout"]) + rin * (o["cin"] | 1) + rout * (o["cout"] | 1), 0)


def _lds_dx(o, rows_dp, rows_dx):
    return _lds_body(o["k"] * _up4(o["cout"]) * _up16(o["cin"]) + rows_dp * (o["cout"] | 1) + rows_dx * (o["cin"] | 1), o["n_src"] - 1)


def _lds_wg(o, rin, rout):
    tasks = o["k"] * o["cin"]
    mt, nt = (tasks + 15) // 16, (o["cout"] + 15) // 16
    b = ((rin * (o["cin"] | 1) + 6) // 4 * 4 + _up4(rout) * _up16(o["cout"])) * 4
    if gwg_kparts(tasks) > 1:
        b = max(b, gwg_kparts(tasks) * mt * nt * 256 * 4)
    return b


def build_graph(ops, frames, head_attention=False, head_pool=0, tabs=None):
    """plan_ops (graph_engine.hip) over the op dicts of a layout: per op its shape, sources, twin_next, planes / pc, adders;
    and of the model inline_ok (the rule g_inline_ok), frame_chunks (the automatic setting) and head2.  ValueError where plan_ops
    refuses ("not instantiated", "exceeds 256", "LDS")."""
    tabs = tabs or tables()
    G = []
    n = len(ops)
    ncons = [0] * n
    for i, s in enumerate(ops):
        srcs = [int(v) for v in s["src"]]
        o = dict(kind=s.get("kind", "conv"), norm=s.get("norm", "bn"), act=s.get("act", "relu"), k=int(s["kernel"]),
                 dil=int(s.get("dilation", 1)), stride=max(1, int(s.get("stride", 1))), cout=int(s["filters"]),
                 groups=int(s.get("bn_groups", 1)), res_src=-1 if s.get("residual") is None else int(s["residual"]),
                 res_drop=int(s.get("residual_drop", 0)), n_src=len(srcs), src=srcs, toff=[int(v) for v in s.get("drop", [0] * len(srcs))],
                 sc0=[], scn=[], cin=0, tin=None, needs_dx=False, adders=[], twin_next=False, planes=1, pc=0)
        sl = list(s.get("slice", [(0, 0)] * len(srcs)))
        for j, src in enumerate(srcs):
            assert -1 <= src < i, (i, src)
            T = frames if src < 0 else G[src]["tout"]
            cfull = FEATURE_BINS if src < 0 else G[src]["cout"]
            c0, C = (int(sl[j][0]), int(sl[j][1])) if sl[j][1] > 0 else (0, cfull)
            rows = T - o["toff"][j]
            assert o["tin"] in (None, rows), (i, "sources are not aligned")
            o["tin"] = rows
            o["cin"] += C
            o["sc0"].append(c0)
            o["scn"].append(C)
            if src >= 0:
                o["needs_dx"] = True
                ncons[src] += 1
        span = o["tin"] - (o["k"] - 1) * o["dil"]
        if span <= 0:
            raise ValueError("op %d: spectrogram too short for the kernel sizes" % i)
        o["tout"] = (span - 1) // o["stride"] + 1
        for key in ("cin", "tin", "tout"):
            assert int(s.get(key, o[key])) == o[key], (i, key, s.get(key), o[key])   # the layout's own bookkeeping
        pad = (o["k"] - 1) * o["dil"]
        if o["kind"] == "depthwise":
            assert o["n_src"] == 1 and o["cin"] == o["cout"] and o["norm"] != "bn"
            if o["cout"] > K_THREADS or o["k"] * o["cout"] > 8 * K_THREADS:
                raise ValueError("op %d: depthwise op too large" % i)
            lds = 0   # (far below the limit at these window lengths)
        else:
            if o["cout"] not in tabs["widths"]:
                raise ValueError("op %d: filter count not instantiated" % i)
            if o["needs_dx"] and o["cin"] not in tabs["widths"]:
                raise ValueError("op %d: input channel count not instantiated" % i)
            if o["k"] * o["cin"] > K_THREADS:
                raise ValueError("op %d: kernel x input channels exceeds 256" % i)
            lds = max(_lds_fwd(o, o["tin"], o["tout"]), _lds_dx(o, o["tout"] + 2 * pad, o["tin"]) if o["needs_dx"] else 0,
                      _lds_wg(o, o["tin"], o["tout"]))
        if lds > K_MAX_DYN_LDS:
            raise ValueError("op %d: window does not fit the LDS tile" % i)
        G.append(o)
    for i, o in enumerate(G):
        if o["res_src"] >= 0:
            G[o["res_src"]]["adders"].append(i)
    # twins: consecutive, mutually independent convolutions of one shape
    for i in range(n - 2):
        a, b = G[i], G[i + 1]
        same = (a["kind"] == "conv" and b["kind"] == "conv" and all(a[f] == b[f] for f in ("k", "dil", "cin", "cout", "groups", "act", "tin"))
                and a["norm"] == "bn" and b["norm"] == "bn" and a["stride"] == 1 and b["stride"] == 1 and a["n_src"] == 1 and b["n_src"] == 1
                and a["src"][0] >= 0 and b["src"][0] >= 0 and b["src"][0] != i and a["res_src"] < 0 and b["res_src"] < 0
                and not a["adders"] and not b["adders"] and a["cin"] == a["cout"] and a["cout"] in tabs["twins"])
        shared = same and a["src"][0] == b["src"][0] and a["sc0"][0] < b["sc0"][0] + b["cin"] and b["sc0"][0] < a["sc0"][0] + a["cin"]
        if same and not shared and (i == 0 or not G[i - 1]["twin_next"]):
            a["twin_next"] = True
    # planar tensors: 30- and 48-filter producers read only as equal channel slices by convolutions
    for pi in range(n - 1):
        pr = G[pi]
        if pr["kind"] != "conv" or pr["norm"] != "bn" or pr["res_src"] >= 0 or pr["adders"] or pr["cout"] not in (30, 48):
            continue
        cn, ok = 0, True
        for i in range(pi + 1, n):
            for j in range(G[i]["n_src"]):
                if G[i]["src"][j] != pi:
                    continue
                if G[i]["kind"] != "conv" or G[i]["res_src"] >= 0 or G[i]["stride"] != 1:
                    ok = False
                if cn == 0:
                    cn = G[i]["scn"][j]
                if G[i]["scn"][j] != cn or G[i]["scn"][j] >= pr["cout"] or G[i]["sc0"][j] % cn:
                    ok = False
        if ok and cn > 0 and pr["cout"] % cn == 0 and cn % 2 == 0:
            pr["planes"], pr["pc"] = pr["cout"] // cn, cn
    inline_ok = True
    for o in G:
        conv_ok = o["kind"] == "conv" and o["norm"] in ("bn", "none")
        dw_ok = o["kind"] == "depthwise" and o["norm"] in ("bias", "none")
        if not (conv_ok or dw_ok) or o["res_src"] >= 0 or o["adders"] or o["cout"] > K_GFOLDC:
            inline_ok = False
    lo = G[-1]
    head2 = lo["tout"] > 1 and bool(head_attention or head_pool)   # GraphModel::layout
    return dict(G=G, frames=int(frames), inline_ok=inline_ok and not head_attention and not head_pool,
                frame_chunks=1 if any(o["kind"] == "depthwise" for o in G) else 0, head2=head2)


# ------------------------------------------------------------------------------------------ dispatch, restated
def make_ctx(model, options=None, tabs=None, lazy=False, B=1, grid=0):
    """What the dispatch reads besides the op: the model of build_graph(), the engine options (defaults of graph_engine.hip), the
    train step's hand-over decision `inl`, and for the gathering stem whether the batch is descriptor-only, B and the grid."""
    o = dict(bn_inline=1, graph_planar=1, graph_static_shapes=1, graph_role_split=1, graph_dgrad_share=50, profile_split=0)
    o.update(options or {})
    fc = o.get("graph_frame_chunks", model["frame_chunks"])
    return dict(model=model, G=model["G"], tabs=tabs or tables(), planar=bool(o["graph_planar"]), static=bool(o["graph_static_shapes"]),
                frame_chunks=int(fc), inl=bool(o["bn_inline"]) and model["inline_ok"] and not o["profile_split"],
                role_split=bool(o["graph_role_split"]), dgrad_share=int(o["graph_dgrad_share"]), profile_split=bool(o["profile_split"]),
                lazy=bool(lazy), B=int(B), grid=int(grid))


def _planes(ctx, o):
    return o["planes"] if ctx["planar"] and o["planes"] > 1 else 1


def shape_id(ctx, o):
    """g_shape_id: the static shape (MWW_G_SHAPES id) of op `o`, or 0."""
    if not ctx["static"] or o["kind"] != "conv" or o["dil"] != 1 or o["stride"] != 1 or o["res_src"] >= 0 or o["n_src"] < 1:
        return 0
    if o["tin"] > K_GTMAX or o["tout"] > K_GTMAX:
        return 0
    C, L = [0, 0, 0], [0, 0, 0]
    for i in range(o["n_src"]):
        if o["src"][i] < 0:
            C[i] = L[i] = FEATURE_BINS
        else:
            pr = ctx["G"][o["src"][i]]
            if pr["res_src"] >= 0:
                return 0
            C[i] = o["scn"][i]
            L[i] = o["scn"][i] if _planes(ctx, pr) > 1 else pr["cout"]
        v = 4 if ((C[i] | L[i]) & 3) == 0 else (2 if ((C[i] | L[i]) & 1) == 0 else 1)
        if o["src"][i] >= 0 and L[i] != C[i] and o["sc0"][i] % v:
            return 0
    want = (o["k"], o["n_src"], C[0], L[0], C[1], L[1], C[2], L[2])
    for sid, row in ctx["tabs"]["shapes"].items():
        if row == want:
            return sid
    return 0


def chunks(ctx, o, backward):
    """g_chunks: (S, Tc) - S frame chunks of Tc output frames per window, S = 1: whole windows."""
    if (not ctx["inl"] or ctx["frame_chunks"] == 0 or o["kind"] != "conv" or o["tout"] < 32
            or (backward and o["needs_dx"] and o["k"] != 1)):
        return 1, o["tout"]
    S = ctx["frame_chunks"]
    if S == 1:
        while S < 4:
            t = (o["tout"] + S - 1) // S
            ti = (t - 1) * o["stride"] + (o["k"] - 1) * o["dil"] + 1
            lds = (max(_lds_wg(o, ti, t), _lds_dx(o, t, t) if o["needs_dx"] else 0) if backward else _lds_fwd(o, ti, t))
            if lds + 3072 <= 40960:
                break
            S += 1
    S = min(S, 4)
    Tc = (o["tout"] + S - 1) // S
    return (S, Tc) if (S - 1) * Tc < o["tout"] else (1, Tc)


def stem_gathers(ctx):
    """g_stem_gathers: exactly one op reads the spectrogram, as its only source, and its shape has a gathering instantiation."""
    G = ctx["G"]
    if ctx["model"]["frames"] > K_GXROWS:
        return False
    readers = [(i, s) for i, o in enumerate(G) for s in range(o["n_src"]) if o["src"][s] < 0]
    if len(readers) != 1:
        return False
    o = G[readers[0][0]]
    if o["n_src"] != 1 or o["toff"][0] != 0 or o["tin"] != ctx["model"]["frames"]:
        return False
    return (shape_id(ctx, o), o["cout"]) in ctx["tabs"]["xg"]


def _gathering_launch(ctx, o, ch):
    """Does the launch of stem `o` gather (launch_gconv / launch_gwgrad: the XG instantiation, unless the grid leaves a
    workgroup more than kXMaxSamples windows - then x is written out first)?  The automatic grid gives every window a workgroup
    up to 4 x the CU count, far above any B of this sweep."""
    if not ctx["lazy"] or ch or not any(s < 0 for s in o["src"]) or not stem_gathers(ctx):
        return False
    if o["n_src"] != 1 or o["tin"] > K_GXROWS:
        return False
    grid = min(ctx["B"], ctx["grid"]) if ctx["grid"] > 0 else ctx["B"]
    return -(-ctx["B"] // grid) <= K_XMAX_SAMPLES


def instantiation(role, op, ctx):
    """The kernel instantiation the launch `role` of op index `op` runs, as its demangled template name, or None where the
    launcher finds none (the engine then takes another route without a word).  Roles: "fwd", "fwd2" (op and op + 1), "bwd"
    (fused), "bwd2" (op - 1 and op), "wgrad", "dgrad", "dw_fwd", "dw_dgrad", "dw_wgrad", "head"."""
    G, tabs = ctx["G"], ctx["tabs"]
    o = G[op]
    if role == "dw_fwd":
        return "gdw_kernel<0>"
    if role == "dw_dgrad":
        return "gdw_kernel<1>"
    if role == "dw_wgrad":
        return "gdw_wgrad_kernel"
    if role == "head":
        return "ghead_att_kernel" if ctx["model"]["head2"] else "ghead_kernel"
    nc = o["cout"]
    if role == "fwd":
        S, _ = chunks(ctx, o, False)
        sid = shape_id(ctx, o) if S == 1 else 0
        if _gathering_launch(ctx, o, S > 1) and (sid, nc) in tabs["xg"]:
            return "gconv_xg_kernel<%d, GSh%d>" % (nc, sid)
        if S == 1 and (sid, nc) in tabs["fwd"]:
            return "gconv_kernel<%d, 0, GSh%d>" % (nc, sid)
        if nc not in tabs["widths"]:
            return None
        return "gconv_chunk_kernel<%d, 0>" % nc if S > 1 else "gconv_kernel<%d, 0>" % nc
    if role == "fwd2":
        s0, s1 = shape_id(ctx, o), shape_id(ctx, G[op + 1])
        sid = s0 if s0 == s1 else 0
        if (sid, nc) in tabs["fwd2"]:
            return "gconv_fwd2_kernel<%d, GSh%d>" % (nc, sid)
        return "gconv_fwd2_kernel<%d>" % nc if nc in tabs["twins"] else None
    if role == "bwd2":
        s0, s1 = shape_id(ctx, o), shape_id(ctx, G[op - 1])
        sid = s0 if s0 == s1 else 0
        if (sid, nc) in tabs["bwd2"]:
            return "gconv_bwd2_kernel<%d, %d, GSh%d>" % (nc, nc, sid)
        return "gconv_bwd2_kernel<%d, %d>" % (nc, nc) if nc in tabs["twins"] else None
    S, _ = chunks(ctx, o, True)
    sid = shape_id(ctx, o) if S == 1 else 0
    if role == "bwd":
        if not o["needs_dx"] or ctx["profile_split"]:
            return None
        if S == 1 and (sid, nc, o["cin"]) in tabs["bwd"]:
            return "gconv_bwd_kernel<%d, %d, GSh%d>" % (nc, o["cin"], sid)
        if (nc, o["cin"]) not in tabs["pairs"]:
            return None
        return ("gconv_bwd_chunk_kernel<%d, %d>" if S > 1 else "gconv_bwd_kernel<%d, %d>") % (nc, o["cin"])
    if role == "wgrad":
        if _gathering_launch(ctx, o, S > 1) and (sid, nc) in tabs["xg"]:
            return "gconv_wgrad_xg_kernel<%d, GSh%d>" % (nc, sid)
        if S == 1 and (sid, nc) in tabs["wg"]:
            return "gconv_wgrad_kernel<%d, GSh%d>" % (nc, sid)
        if nc not in tabs["widths"]:
            return None
        return "gconv_wgrad_chunk_kernel<%d>" % nc if S > 1 else "gconv_wgrad_kernel<%d>" % nc
    if role == "dgrad":
        if o["cin"] not in tabs["widths"]:
            return None
        return ("gconv_chunk_kernel<%d, 1>" if S > 1 else "gconv_kernel<%d, 1>") % o["cin"]
    raise ValueError(role)


def train_step_launches(ctx):
    """[(profile name, [instantiations], role, op index)] of one train step, in launch order: enqueue_forward(training) and
    enqueue_backward of graph_engine.hip.  The profile names are those Launcher::begin records under option "profile"."""
    G, inl = ctx["G"], ctx["inl"]
    n = len(G)
    out = []
    i = 0
    while i < n:
        o = G[i]
        if o["kind"] == "depthwise":
            out.append(("dw_fwd%d" % (i + 1), [instantiation("dw_fwd", i, ctx)], "dw_fwd", i))
            i += 1
            continue
        if o["twin_next"] and not ctx["profile_split"] and instantiation("fwd2", i, ctx):
            out.append(("conv_fwd2_%d" % (i + 1), [instantiation("fwd2", i, ctx)], "fwd2", i))
            if not inl:
                out.append(("bn_fwd_finalize2_%d" % (i + 1), ["gbn_fwd_finalize2_kernel"], "fin", i))
            i += 2
            continue
        k = instantiation("fwd", i, ctx)
        if k is None:
            raise ValueError("op %d: conv width not instantiated" % i)
        out.append(("conv_fwd%d" % (i + 1), [k], "fwd", i))
        if o["norm"] == "bn" and not inl:
            out.append(("bn_fwd_finalize%d" % (i + 1), ["gbn_fwd_finalize_kernel"], "fin", i))
        i += 1
    out.append(("head", [instantiation("head", n - 1, ctx)], "head", n - 1))
    i = n - 1
    while i >= 0:
        o = G[i]
        if i > 0 and G[i - 1]["twin_next"] and not ctx["profile_split"]:
            k = instantiation("bwd2", i, ctx)
            if k is None:
                raise ValueError("twin ops without a fused backward instantiation")
            out.append(("conv_bwd2_%d" % (i + 1), ([] if inl else ["gbn_bwd_finalize2_kernel"]) + [k], "bwd2", i))
            i -= 2
            continue
        if o["adders"]:
            out.append(("residual_gather%d" % (i + 1), ["gres_gather_kernel"], "res", i))
        if o["norm"] == "bn" and not inl:
            out.append(("bn_bwd_finalize%d" % (i + 1), ["gbn_bwd_finalize_kernel"], "fin", i))
        elif o["norm"] == "bias" and not inl:
            out.append(("bias_grad%d" % (i + 1), ["gbn_bwd_finalize_kernel"], "fin", i))
        if o["kind"] == "depthwise":
            out.append(("dw_wgrad%d" % (i + 1), [instantiation("dw_wgrad", i, ctx)], "dw_wgrad", i))
            if o["needs_dx"]:
                out.append(("dw_dgrad%d" % (i + 1), [instantiation("dw_dgrad", i, ctx)], "dw_dgrad", i))
            i -= 1
            continue
        k = instantiation("bwd", i, ctx)
        if k is not None:
            out.append(("conv_bwd%d" % (i + 1), [k], "bwd", i))
        else:
            k = instantiation("wgrad", i, ctx)
            if k is None:
                raise ValueError("op %d: conv width not instantiated" % i)
            out.append(("conv_wgrad%d" % (i + 1), [k], "wgrad", i))
            if o["needs_dx"]:
                k = instantiation("dgrad", i, ctx)
                if k is None:
                    raise ValueError("op %d: conv width not instantiated" % i)
                out.append(("conv_dgrad%d" % (i + 1), [k], "dgrad", i))
        i -= 1
    return out


def eval_forward_kernels(ctx):
    """Kernels of a forward pass outside the train step (check_graph_mixednet's forward taps: evaluation and training mode
    without the hand-over's chunks differ from the step's only in gbn_eval_prepare_kernel and whole-window forms)."""
    e = dict(ctx, inl=False)
    ks = {k for _, kk, role, _ in train_step_launches(e) if role in ("dw_fwd", "fwd", "fwd2", "head") for k in kk}
    if any(o["norm"] == "bn" for o in ctx["G"]):
        ks.add("gbn_eval_prepare_kernel")
    return ks


# ------------------------------------------------------------------------------------------ inventory
_PLAIN = ("gdw_kernel<0>", "gdw_kernel<1>", "gdw_wgrad_kernel", "gres_gather_kernel", "ghead_kernel", "ghead_att_kernel",
          "gbn_fwd_finalize_kernel", "gbn_fwd_finalize2_kernel", "gbn_bwd_finalize_kernel", "gbn_bwd_finalize2_kernel",
          "gbn_eval_prepare_kernel")


def inventory(tabs=None):
    """Every instantiation the launchers of tu_graph.hip and graph_engine.hip can reach."""
    t = tabs or tables()
    inv = set(_PLAIN)
    for n in t["widths"]:
        inv |= {"gconv_kernel<%d, 0>" % n, "gconv_kernel<%d, 1>" % n, "gconv_chunk_kernel<%d, 0>" % n, "gconv_chunk_kernel<%d, 1>" % n,
                "gconv_wgrad_kernel<%d>" % n, "gconv_wgrad_chunk_kernel<%d>" % n}
    inv |= {"gconv_kernel<%d, 0, GSh%d>" % (n, s) for s, n in t["fwd"]}
    inv |= {"gconv_fwd2_kernel<%d, GSh%d>" % (n, s) for s, n in t["fwd2"]}
    inv |= {"gconv_wgrad_kernel<%d, GSh%d>" % (n, s) for s, n in t["wg"]}
    inv |= {"gconv_xg_kernel<%d, GSh%d>" % (n, s) for s, n in t["xg"]} | {"gconv_wgrad_xg_kernel<%d, GSh%d>" % (n, s) for s, n in t["xg"]}
    inv |= {"gconv_bwd_kernel<%d, %d, GSh%d>" % (a, b, s) for s, a, b in t["bwd"]}
    inv |= {"gconv_bwd2_kernel<%d, %d, GSh%d>" % (n, n, s) for s, n in t["bwd2"]}
    for a, b in t["pairs"]:
        inv |= {"gconv_bwd_kernel<%d, %d>" % (a, b), "gconv_bwd_chunk_kernel<%d, %d>" % (a, b)}
    for n in t["twins"]:
        inv |= {"gconv_fwd2_kernel<%d>" % n, "gconv_bwd2_kernel<%d, %d>" % (n, n)}
    return frozenset(inv)


def launcher_of(inst):
    """The launcher template of an instantiation; the MODE of gconv_kernel / gconv_chunk_kernel / gdw_kernel stays in the name
    (forward and data gradient are different code)."""
    name, _, args = inst.partition("<")
    if name in ("gconv_kernel", "gconv_chunk_kernel"):
        return "%s<N, %s>" % (name, args.rstrip(">").split(", ")[1])
    if name == "gdw_kernel":
        return inst
    return name


def _grid_anchors(tabs):
    a = set()
    for co, ci in tabs["pairs"]:
        a |= {"gconv_bwd_kernel<%d, %d>" % (co, ci), "gconv_bwd_chunk_kernel<%d, %d>" % (co, ci)}
    for n in tabs["widths"]:
        a |= {"gconv_wgrad_kernel<%d>" % n, "gconv_wgrad_chunk_kernel<%d>" % n, "gconv_kernel<%d, 1>" % n, "gconv_chunk_kernel<%d, 1>" % n}
    return a


def _is_chunk(inst):
    return "_chunk_kernel" in inst


def required(tabs=None):
    """What the plan must cover: the inventory and the axis items of the module docstring."""
    t = tabs or tables()
    inv = inventory(t)
    req = set(inv)
    for inst in _grid_anchors(t):
        req |= {("auto", inst), ("grid2", inst)}
    req |= {("dgrad-share", v) for v in (10, 30, 90)} | {("B<grid",)}
    req |= {("S", i, s) for i in inv if _is_chunk(i) for s in (2, 3, 4)} | {("short-chunk", s) for s in (2, 3, 4)}
    req |= {("tout", v) for v in (31, 32, 33)} | {("auto-chunks", 3)}
    req |= {("kparts", p, f) for p in (4, 2, 1) for f in ("fused", "split")}
    req |= {("dw-taps", k) for k in (1, 8, 9, 16, 17)} | {("dw-ch", c) for c in (16, 32, 64, 24, 40, 48)}
    req |= {("dw-bias", True), ("dw-bias", False), ("dw-mix1",)}
    req |= {("ssn", g, h) for g in (1, 2, 4) for h in ("handover", "finalize")} | {("twin-finalize2",)}
    req |= {("static", p, f, T) for p in (1, 0) for f in (True, False) for T in (208, 212)}
    req |= {("gather", 200), ("gather", 201), ("gather", "overflow")}
    req |= {("head", h) for h in ("att", "avg", "max", "att+pool")} | {("residual-two-adders",)}
    return frozenset(req)


# ------------------------------------------------------------------------------------------ cases
def case_layout(case):
    from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout
    if case["kind"] == "mixednet":
        return GraphMixedNetLayout(case["flags"], case["T"])
    return InceptionLayout(case["flags"], case["T"], fuse_heads=case["fuse_heads"])


def case_ctx(case, tabs=None, sync_bn=False):
    """`sync_bn`: the case as a rank of a sync-BN data-parallel step (GWalk of graph_engine.hip with an exchange hook that
    reduces the statistics): no statistics hand-over - every BatchNorm takes its finalize launches, behind the exchange - and
    "pairing off" - twin ops launch singly, forward and backward."""
    lay = case_layout(case)
    model = build_graph(lay.ops, case["T"], getattr(lay, "head_attention", False), getattr(lay, "head_pool", 0), tabs)
    lazy = case["kind"] == "gather"
    options = case["options"]
    if sync_bn:
        options = dict(options, bn_inline=0)
        model = dict(model, G=[dict(o, twin_next=False) for o in model["G"]])
    return make_ctx(model, options, tabs, lazy=lazy, B=case["B"], grid=case["grid"])


def case_route(case, tabs=None, sync_bn=False):
    """The graph engine's launch names of the case's train step, as option "profile" records them."""
    return [name for name, _, _, _ in train_step_launches(case_ctx(case, tabs, sync_bn))]


def case_kernels(case, tabs=None, sync_bn=False):
    """The instantiations the case's train step launches, in launch order."""
    return [k for _, ks, _, _ in train_step_launches(case_ctx(case, tabs, sync_bn)) for k in ks]


ROUTE_PREFIXES = ("conv_fwd", "conv_bwd", "conv_wgrad", "conv_dgrad", "dw_fwd", "dw_wgrad", "dw_dgrad", "bn_fwd_finalize", "bn_bwd_finalize",
                  "bias_grad", "residual_gather", "bn_eval_prepare", "head")


def route_of_profile(names):
    """The graph engine's own launches among the names mww_profile_read returns (the rest: batch assembly, metrics and the
    dense-weight gradient, gradient assembly and Adam belong to the shared core)."""
    return [n for n in names if n.startswith(ROUTE_PREFIXES) and not n.startswith("head_tail")]


def case_items(case, tabs=None):
    """What a case covers (the terms of required())."""
    t = tabs or tables()
    ctx = case_ctx(case, t)
    G = ctx["G"]
    launches = train_step_launches(ctx)
    items = {k for _, ks, _, _ in launches for k in ks}
    opt, flags = case["options"], case["flags"]
    if case["kind"] == "gather":
        T = case["T"]
        if T <= K_GXROWS and "gconv_xg_kernel<24, GSh1>" not in items:
            items.add(("gather", "overflow"))
        else:
            items.add(("gather", T))
        return items   # (compared with the materialised batch, not with the oracle: counts for nothing else)
    if case["kind"] == "mixednet":
        items |= eval_forward_kernels(ctx) & {"gbn_eval_prepare_kernel"}
    anchors = _grid_anchors(t)
    fc_opt = opt.get("graph_frame_chunks")
    gridmode = "auto" if case["grid"] == 0 else ("grid2" if (case["grid"], case["B"]) == (2, 5) else None)
    if case["grid"] > case["B"]:
        items.add(("B<grid",))
    for name, ks, role, i in launches:
        o = G[i]
        for k in ks:
            if k in anchors and gridmode and ctx["inl"] and ctx["role_split"]:
                items.add((gridmode, k))
            if _is_chunk(k):
                S = chunks(ctx, o, role != "fwd")[0]
                if fc_opt in (2, 3, 4):
                    items.add(("S", k, S))
                    if o["tout"] % S:
                        items.add(("short-chunk", S))
                elif S > 1:
                    items.add(("auto-chunks", S))
        if role == "bwd" and ctx["inl"] and ctx["role_split"] and case["grid"] == 0 and opt.get("graph_dgrad_share", 50) != 50:
            items.add(("dgrad-share", opt["graph_dgrad_share"]))
        if role in ("bwd", "wgrad") and ks[0].split("<")[0] in ("gconv_bwd_kernel", "gconv_bwd_chunk_kernel", "gconv_wgrad_kernel", "gconv_wgrad_chunk_kernel"):
            items.add(("kparts", gwg_kparts(o["k"] * o["cin"]), "fused" if role == "bwd" else "split"))
        if role == "fwd" and fc_opt in (2, 3, 4) and ctx["inl"] and o["tout"] in (31, 32, 33) and (o["tout"] >= 32) == _is_chunk(ks[0]):
            items.add(("tout", o["tout"]))   # (31: the whole-window kernel; 32, 33: chunks)
        if role == "dw_fwd":
            items |= {("dw-taps", o["k"]), ("dw-ch", o["cout"]), ("dw-bias", o["norm"] == "bias")}
        if role in ("fwd", "fwd2") and o["norm"] == "bn" and case["kind"] == "inception":
            items.add(("ssn", o["groups"], "handover" if ctx["inl"] else "finalize"))
        if name.startswith("bn_fwd_finalize2_") and any(n2.startswith("conv_bwd2_") and "gbn_bwd_finalize2_kernel" in k2 for n2, k2, _, _ in launches):
            items.add(("twin-finalize2",))
        if role == "res" and len(o["adders"]) == 2:
            items.add(("residual-two-adders",))
    if case["kind"] == "mixednet":
        if any(1 in g and len(g) > 1 for g in mo.parse(flags["mixconv_kernel_sizes"]) if isinstance(g, (list, tuple))):
            items.add(("dw-mix1",))
        if ctx["model"]["head2"]:
            att, pool = bool(flags.get("spatial_attention")), bool(flags.get("pooled"))
            items.add(("head", "att+pool" if att and pool else ("att" if att else ("max" if flags.get("max_pool") else "avg"))))
    if case["kind"] == "inception" and all(flags[k] == v for k, v in mo.INCEPTION_DEFAULTS.items()):
        items.add(("static", int(opt.get("graph_planar", 1)), bool(case["fuse_heads"]), case["T"]))
    return items


def describe(case):
    return "%s: %s %s T %d B %d grid %d options %s%s seed %d; route %s" % (
        case["id"], case["kind"], {k: v for k, v in case["flags"].items()
                                   if (mo.MIXEDNET_DEFAULTS if case["kind"] == "mixednet" else mo.INCEPTION_DEFAULTS).get(k) != v},
        case["T"], case["B"], case["grid"], case["options"], "" if case["fuse_heads"] else " unfused heads", case["seed"],
        " ".join(case_route(case)))


# ------------------------------------------------------------------------------------------ plan
def _mixednet_flags(f0, widths, kernels, k0=3, stride=1, repeat=None, residual=None, **extra):
    n = len(widths)
    one = n == 1   # (a one-element list is written with a trailing comma, as the fuzz's flag sets are)
    return dict(mo.MIXEDNET_DEFAULTS, pointwise_filters=",".join(map(str, widths)) + ("," if one else ""),
                repeat_in_block=",".join(map(str, repeat or [1] * n)) + ("," if one else ""),
                residual_connection=",".join(map(str, residual or [0] * n)) + ("," if one else ""),
                mixconv_kernel_sizes=",".join(str(list(k)) for k in kernels) + ("," if one else ""),
                first_conv_filters=f0, first_conv_kernel_size=k0, stride=stride, **extra)


def _case(cid, kind, flags, T, B, grid, options=None, fuse_heads=True, seed=42):
    return dict(id=cid, kind=kind, flags=flags, T=int(T), B=int(B), grid=int(grid), options=dict(options or {}), fuse_heads=bool(fuse_heads), seed=int(seed))


def near_zero_count(case):
    """engine_checks.count_graph_mixednet_near_zero of a MixedNet case (0 for the others: check_inception_train_steps imposes
    the engine's own ReLU decisions on the oracle)."""
    if case["kind"] != "mixednet":
        return 0
    import engine_checks as ec
    return ec.count_graph_mixednet_near_zero(case["flags"], case["B"], case["T"], steps=1, seed=case["seed"])


def _well_posed(case):
    """MIN_FINAL_FRAMES / MIN_BN_ROWS of the case's graph."""
    G = case_ctx(case)["G"]
    if G[-1]["tout"] < MIN_FINAL_FRAMES:
        return False
    return all(case["B"] * o["tout"] * (o["cout"] // o["groups"] if o["groups"] > 1 else 1) >= MIN_BN_ROWS for o in G if o["norm"] == "bn")


class _Planner:
    def __init__(self, seed, tabs):
        self.rng = random.Random(seed)
        self.tabs = tabs
        self.need = set(required(tabs)) - set(UNREACHABLE)
        self.cases = []

    def add(self, case):
        assert _well_posed(case), describe(case)
        if case["kind"] == "mixednet":   # no unit at a ReLU zero / attention tie: redraw the seed
            for _ in range(20):
                if near_zero_count(case) == 0:
                    break
                case["seed"] += 1
            else:
                raise RuntimeError("no seed without a near-zero unit: " + describe(case))
        got = case_items(case, self.tabs)
        self.need -= got
        self.cases.append(case)
        return got

    # ---- MixedNet chains: conv1 (40 -> f0, never a data gradient: weight-gradient launch) and three 1x1 ops (cin -> cout: fused
    # pair or weight-gradient + data-gradient launches) behind 3-tap depthwise ops
    def _op_gain(self, cout, cin, chunk, gridmode, S):
        t = self.tabs
        ks = ["gconv_chunk_kernel<%d, 0>" % cout if chunk else "gconv_kernel<%d, 0>" % cout]
        if (cout, cin) in t["pairs"]:
            ks.append(("gconv_bwd_chunk_kernel<%d, %d>" if chunk else "gconv_bwd_kernel<%d, %d>") % (cout, cin))
        else:
            ks += [("gconv_wgrad_chunk_kernel<%d>" if chunk else "gconv_wgrad_kernel<%d>") % cout,
                   ("gconv_chunk_kernel<%d, 1>" if chunk else "gconv_kernel<%d, 1>") % cin]
        g = 0
        for k in ks:
            g += (k in self.need) + ((gridmode, k) in self.need) + (("S", k, S) in self.need)
        return g

    def _stem_gain(self, f0, chunk, gridmode, S):
        ks = ["gconv_chunk_kernel<%d, 0>" % f0 if chunk else "gconv_kernel<%d, 0>" % f0,
              "gconv_wgrad_chunk_kernel<%d>" % f0 if chunk else "gconv_wgrad_kernel<%d>" % f0]
        return sum((k in self.need) + ((gridmode, k) in self.need) + (("S", k, S) in self.need) for k in ks)

    def chain(self, chunk, S, gridmode):
        """One three-block MixedNet of the largest gain under (form, grid mode), or None when nothing is left for it."""
        rng, ws = self.rng, self.tabs["widths"]
        best = max(((self._stem_gain(f0, chunk, gridmode, S) + self._op_gain(w1, f0, chunk, gridmode, S), rng.random(), f0, w1)
                    for f0 in ws for w1 in ws))
        total, _, f0, w1 = best
        if total == 0:
            return None
        widths = [w1]
        while len(widths) < 3:
            g, _, w = max((self._op_gain(w, widths[-1], chunk, gridmode, S), rng.random(), w) for w in ws)
            if g == 0:
                break
            widths.append(w)
        nb = len(widths)
        # frames: conv1 and every depthwise op take 2; a chunked case keeps 32 or more to the end, the others MIN_FINAL_FRAMES and more
        T = max(40, (32 if chunk else 24) + 2 * (nb + 1) + rng.randrange(1, 8))
        B = 5 if gridmode == "grid2" else rng.randint(3, 6)
        opts = {"graph_frame_chunks": S if chunk else 0}
        if not chunk and any((a, b) in ((30, 24), (30, 10), (48, 10)) for a, b in zip(widths, [f0] + widths)):
            opts["graph_static_shapes"] = 0   # (a 1x1 op over 24 or 10 whole channels has the static shape of Inception's fused heads)
        form = "chunk%d" % S if chunk else "whole"
        anchor = ("pair%dx%d" if (w1, f0) in self.tabs["pairs"] else "pw%dx%d") % (w1, f0)
        return _case("%s-%s-%s" % (anchor, "%s" % form if (w1, f0) in self.tabs["pairs"] else "split-" + form, gridmode),
                     "mixednet", _mixednet_flags(f0, widths, [[3]] * nb), T, B, 0 if gridmode == "auto" else 2, opts)


def _inception_flags(stem, stem_k, stem_g, f1, f2, k, g, dil, dropout=0.2):
    j = lambda v: ",".join(map(str, v))   # noqa: E731
    return dict(cnn1_filters=j(stem), cnn1_kernel_sizes=j(stem_k), cnn1_subspectral_groups=j(stem_g), cnn2_filters1=j(f1), cnn2_filters2=j(f2),
                cnn2_kernel_sizes=j(k), cnn2_subspectral_groups=j(g), cnn2_dilation=j(dil), dropout=dropout)


@functools.lru_cache(maxsize=None)
def _plan(seed, path):
    tabs = tables(path)
    p = _Planner(seed, tabs)
    INC = dict(mo.INCEPTION_DEFAULTS)
    # 1. static shapes: the default Inception flags, planar tensors on / off, fused / unfused heads, on both sides of kGTmax
    for T in (208, 212):
        for planar in (1, 0):
            for fuse in (True, False):
                p.add(_case("static-T%d-%s-%s" % (T, "planar" if planar else "rows", "fused" if fuse else "unfused"), "inception", INC, T, 4, 0,
                            {"graph_planar": planar}, fuse))
    # (the single-op forward instantiations of the twins' static shapes: "profile_split" keeps every op in launches of its own)
    p.add(_case("static-T120-rows-fused-profile-split", "inception", INC, 120, 4, 2, {"graph_planar": 0, "profile_split": 1}, True))
    # 2. twins of every reachable width off the static shapes (3 taps, or dilation 2), SSN groups 1 / 2 / 4 through the hand-over
    # and through the finalize launches, second stem layers (dense k > 1 with a data gradient: the halo path), a frame-chunked
    # Inception (k > 1 forward chunks), fused and unfused heads.  (width, k, dilation, block groups, stems, stem kernels, stem
    # groups, filters2, fuse_heads, bn_inline, grid, B, T, more options)
    inc = [(8, 3, 1, 1, [16], [3], [1], 8, True, 1, 0, 4, 60, {}),
           (10, 3, 2, 2, [24], [5], [2], 10, True, 1, 2, 5, 64, {}),
           (12, 5, 1, 4, [8, 24], [3, 3], [4, 4], 12, True, 1, 0, 3, 70, {}),
           (16, 3, 1, 1, [32], [3], [1], 16, True, 0, 2, 5, 56, {}),
           (20, 5, 2, 2, [20], [3], [2], 20, True, 0, 0, 4, 72, {}),
           (12, 3, 1, 4, [16], [5], [4], 24, True, 0, 8, 3, 60, {}),
           (10, 5, 1, 1, [12, 24], [3, 5], [1, 1], 30, True, 1, 0, 4, 90, {"graph_frame_chunks": 2}),
           (16, 5, 1, 1, [40], [3], [1], 36, False, 1, 0, 4, 64, {"graph_static_shapes": 0}),
           (20, 3, 1, 1, [64], [3], [1], 40, True, 1, 2, 5, 60, {})]
    for w, k, d, g, stems, sk, sg, f2, fuse, inline, grid, B, T, more in inc:
        flags = _inception_flags(stems, sk, sg, [w], [f2], [k], [g], [d])
        opts = dict(more)
        if not inline:
            opts["bn_inline"] = 0
        p.add(_case("twin%d-k%dd%d-g%d-%s" % (w, k, d, g, "handover" if inline else "finalize"), "inception", flags, T, B, grid, opts, fuse))
    # 3. the gathering stem: kGXRows and kXMaxSamples (compared with the materialised batch: check_inception_gathered_stem)
    p.add(_case("gather-T200", "gather", INC, 200, 6, 0))
    p.add(_case("gather-T201", "gather", INC, 201, 6, 0))
    p.add(_case("gather-T200-overflow", "gather", INC, 200, 9, 1))
    # 4. heads and residual branches (finalize launches: such graphs have no hand-over)
    for tag, extra in (("att", dict(spatial_attention=1)), ("avg", dict(pooled=1)), ("max", dict(pooled=1, max_pool=1)),
                       ("att-pool", dict(spatial_attention=1, pooled=1))):
        p.add(_case("head-" + tag, "mixednet", _mixednet_flags(16, [24, 32], [[5], [7]], **extra), 48, 4, 2))
    p.add(_case("residual-two-adders", "mixednet", _mixednet_flags(16, [24, 32], [[5], [3]], repeat=[2, 1], residual=[1, 0]), 52, 4, 2))
    # 5. depthwise ops: taps across the kGDwJ = 8 register blocks, channels that divide 256 and that do not, a 1-tap MixConv group
    p.add(_case("dw-taps8-9-16", "mixednet", _mixednet_flags(16, [32, 64, 8], [[8], [9], [16]]), 58, 4, 0))
    p.add(_case("dw-taps17-mix1", "mixednet", _mixednet_flags(24, [40, 48, 8], [[17], [1, 9], [3, 5]]), 56, 3, 2))
    # 6. the chunk threshold: final frames 31, 32, 33 under "graph_frame_chunks" 2; the automatic setting's 40 KB rule
    for tout in (31, 32, 33):
        p.add(_case("tout%d-chunk2" % tout, "mixednet", _mixednet_flags(16, [24], [[6]], k0=5), tout + 9, 4, 0, {"graph_frame_chunks": 2}))
    p.add(_case("auto-chunks-64x64", "mixednet", _mixednet_flags(32, [64, 64], [[3], [5]]), 104, 3, 0))
    # 7. "graph_dgrad_share" and B below the grid on a fused pair
    for share in (10, 30, 90):
        p.add(_case("pair48x48-share%d" % share, "mixednet", _mixednet_flags(48, [48, 32], [[3], [3]]), 40, 5, 0,
                    {"graph_dgrad_share": share, "graph_frame_chunks": 0}))
    p.add(_case("pair16x16-B3-grid8", "mixednet", _mixednet_flags(16, [16, 24], [[3], [3]]), 40, 3, 8, {"graph_frame_chunks": 0}))
    # 8. every width in every role and form, every fused pair, under per-launch grids and under grid 2 with B = 5
    for S in (0, 2, 3, 4):
        for gridmode in ("auto", "grid2"):
            while True:
                c = p.chain(S > 0, S, gridmode)
                if c is None:
                    break
                before = len(p.need)
                p.add(c)
                if len(p.need) == before:   # (the estimate of chain() and case_items() disagree: stop instead of looping)
                    raise RuntimeError("planner made no progress: " + describe(c))
    seen = {}
    for c in p.cases:
        k = seen.get(c["id"], 0)
        seen[c["id"]] = k + 1
        if k:
            c["id"] += "-%d" % k
    return tuple(p.cases), frozenset(p.need)


def plan(seed=2026, path=LAUNCH_H):
    """The sweep: a list of cases, each a dict (id, kind "inception" / "mixednet" / "gather", flags, T, B, grid, options,
    fuse_heads, seed)."""
    return [dict(c, flags=dict(c["flags"]), options=dict(c["options"])) for c in _plan(seed, path)[0]]


def uncovered(seed=2026, path=LAUNCH_H):
    """Items of required() that plan() does not cover: UNREACHABLE when the plan is complete."""
    tabs = tables(path)
    cov = set()
    for c in plan(seed, path):
        cov |= case_items(c, tabs)
    return sorted(set(required(tabs)) - cov, key=str)


def emulator_slice(seed=2026, path=LAUNCH_H):
    """A fixed slice of the plan for the emulated kernels: every launcher template (launcher_of) at least once, greedily,
    cheapest case first among equals."""
    tabs = tables(path)
    cases = plan(seed, path)
    items = {c["id"]: {launcher_of(k) for k in case_items(c, tabs) if isinstance(k, str)} for c in cases}
    cost = {c["id"]: c["B"] * c["T"] * len(case_ctx(c, tabs)["G"]) * (3 if c["kind"] == "gather" else 1) for c in cases}
    todo = set().union(*items.values())
    out = []
    while todo:
        best = max(cases, key=lambda c: (len(items[c["id"]] & todo) / cost[c["id"]], -cost[c["id"]]))
        out.append(best)
        todo -= items[best["id"]]
    return out


# ------------------------------------------------------------------------------------------ running a case
def run_case(lib, case, strict=True):
    """One train step of the case against the float64 oracle at the bounds of engine_checks (MixedNet: with the forward taps,
    and the looser gradient bound an assertion failure), then the route check."""
    import engine_checks as ec
    try:
        if case["kind"] == "mixednet":
            ec.check_graph_mixednet(lib, case["flags"], B=case["B"], T=case["T"], steps=1, grid=case["grid"], options=case["options"],
                                    seed=case["seed"], strict=strict)
        elif case["kind"] == "inception":
            ec.check_inception_train_steps(lib, B=case["B"], T=case["T"], steps=1, grid=case["grid"], flags=case["flags"],
                                           fuse_heads=case["fuse_heads"], options=case["options"])
        else:
            ec.check_inception_gathered_stem(lib, cases=1, first=0, B=case["B"], lengths=(case["T"],), grid=case["grid"], rounds=1)
            return
        got = profiled_route(lib, case)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (describe(case), e)) from None
    want = case_route(case)
    assert got == want, "%s\nprofiled route %s" % (describe(case), " ".join(got))


def profiled_route(lib, case):
    """The graph engine's launch names of one more train step of the case under option "profile" 1, in an engine of its own set
    up as the checks set theirs up (the profile brackets are event records around unchanged launches; the option itself only
    moves the metrics and the dense-weight gradient onto the main stream)."""
    import numpy as np
    import engine_checks as ec
    from microwakeword_amd import native
    lay = case_layout(case)
    eng = native.Engine(lib=lib, **lay.engine_args(case["B"]))
    try:
        if case["grid"]:
            for k in ("grid_graph", "grid_head"):
                eng.set_option(k, case["grid"])
        for k, v in case["options"].items():
            eng.set_option(k, v)
        eng.set_option("profile", 1)
        rng = np.random.default_rng(5)
        B = case["B"]
        eng.set_batch(ec.synth_x(rng, B, case["T"]))
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), np.ones(B, np.float32))
        if case["kind"] == "inception":
            eng.set_dropout_mask(np.ones((B, lay.t_last * lay.c_last), np.float32))
        eng.train_step(B, 1e-3)
        return route_of_profile([n for n, _ in eng.profile_read()])
    finally:
        eng.close()
