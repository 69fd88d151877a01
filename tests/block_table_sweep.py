"""A covering sweep of the specialised block kernels (csrc/block_launch.hip.h), shared by the GPU sweep
(tests/test_block_table_sweep_gpu.py), its CPU-side checks (tests/test_engine_emulated.py) and tools/table_sweep_kernels.py.

The kernels are fully unrolled templates: one compiled kernel per (shape, form), roughly 700 of them.  A bug tied to one
(cin, cout, K, LAST) or to one tail length sits in a kernel that a handful of sampled topologies never launches, so:

- ``inventory(lib)`` reads the shape table from the built library itself (``block_kernels_cover`` probed over a candidate
  space larger than the table) and expands it with ``instantiation()`` - the launchers' form rules restated in Python - into
  the set of kernel instantiations the library can launch, named as their demangled templates;
- ``plan(lib)`` is a deterministic, seeded list of small train-step cases that launches every one of them at least once,
  every strided first block once in tail mode and once over two 64-row tiles;
- each case runs through ``engine_checks.check_train_steps`` (one step against the float64 oracle)."""
import functools
import itertools
import random

from oracle import model_oracle as mo

TT = 64   # first-conv output rows per time tile (common.hip.h)
MODES = (0, 1, 2)   # 0 = fp32, 1 = bf16 operands of the 1x1 contractions ("pointwise_bf16"), 2 = and bf16 p_k / g_k ("storage_bf16")
MODE_NAME = {0: "fp32", 1: "bf16", 2: "bf16st"}
# engine options that choose between forms (mww_lib.hip; make_engine passes them on), with the library's defaults
OPTION_DEFAULTS = dict(bwd_wide=1, conv1_x6=1, conv1_x6_fwd=0, bwd_first_wide=0)
# blocks per model (first block included), (fp32, bf16 modes): the bf16 modes' own rounding noise grows with depth (a rounding
# flip perturbs the next block's operands enough to flip more) - at five blocks and these short windows the float32 and the
# float64 oracle alone differ by up to 3e-3 in the loss, beyond check_train_steps' bf16 bound (1e-3); at three blocks, B = 8,
# the emulated kernels met every bound in 335 of 336 bf16 cases over six other plan seeds and in all of this plan's
MAX_BLOCKS = (5, 3)
# Conditioning of the comparison, not of the kernels: the last block's BatchNorm normalises over B x (final frames) values per
# channel - over one value (B = 1, one final frame) x - mean is rounding noise that rstd = 1 / sqrt(eps) magnifies 30-fold, and a
# dense layer over two frames averages no operand noise away.  Cases keep at least MIN_FINAL_FRAMES final frames (fp32, bf16
# modes) and, in fp32, MIN_BN_ROWS BN rows; the bf16 cases run B = 8 (the bounds of check_train_steps for the bf16 modes assume
# operand-rounding noise that averages out over the windows of the loss: at fewer, the float32 and the float64 oracle alone
# differ by more than the loss bound now and then).
MIN_FINAL_FRAMES = (8, 24)
MIN_BN_ROWS = 32

# candidate space of the probe: wider than the table on every axis
_CONV1_KERNELS = range(1, 8)
_WIDTHS = range(16, 81, 8)
_DW_KERNELS = range(1, 26)
_STRIDES = range(1, 5)


# ------------------------------------------------------------------------------------------ inventory
def _first_covered(lib, k1, c1, co, k, s, bf16):
    """Is (conv1 kernel, conv1 filters, pointwise filters, depthwise kernel, stride) a first-block shape?  A two-block probe whose
    second block is (co, co, 3); mww_block_kernels_cover checks the first block before any other, so a refusal that does not name
    the first block means the first block passed (the second block or the head may still be outside the table)."""
    ok, why = lib.block_kernels_cover(frames=k1 + s * (k + 8), conv1_filters=c1, conv1_kernel=k1, conv1_stride=s,
                                      block_filters=(co, co), block_kernel=(k, 3), bf16=bf16)
    return ok or not why.startswith("first block")


def _block_covered(lib, first, ci, co, k, bf16):
    """Is (cin, cout, depthwise kernel) a block shape?  A two-block probe behind a known first block of pointwise width ci;
    the head check comes last, so a refusal that does not name block 1 means block 1 passed."""
    k1, c1, _, k0, s = first
    ok, why = lib.block_kernels_cover(frames=k1 + s * (k0 + k + 8), conv1_filters=c1, conv1_kernel=k1, conv1_stride=s,
                                      block_filters=(ci, co), block_kernel=(k0, k), bf16=bf16)
    return ok or not why.startswith("block 1 ")


@functools.lru_cache(maxsize=None)
def _tables(lib):
    """{bf16: (first shapes, block shapes)} as the library's shape table holds them."""
    out = {}
    for bf16 in (False, True):
        firsts = [(k1, c1, co, k, s) for k1, c1, co, k, s in itertools.product(_CONV1_KERNELS, _WIDTHS, _WIDTHS, _DW_KERNELS, _STRIDES)
                  if _first_covered(lib, k1, c1, co, k, s, bf16)]
        anchor = {}
        for f in firsts:
            anchor.setdefault(f[2], f)
        # a block whose input width no first block produces is out of reach of a MixedNet behind these first blocks
        blocks = [(ci, co, k) for ci, co, k in itertools.product(_WIDTHS, _WIDTHS, _DW_KERNELS)
                  if ci in anchor and _block_covered(lib, anchor[ci], ci, co, k, bf16)]
        out[bf16] = (tuple(firsts), tuple(blocks))
    return out


def tables(lib):
    return _tables(lib)


def _b(v):
    return "true" if v else "false"


def instantiation(kind, shape, mode, options, last=False):
    """The kernel instantiation a launcher runs for `shape` in `mode` (0 / 1 / 2) under engine `options` (OPTION_DEFAULTS
    completed), as its demangled template name.  The form rules of mww_lib.hip launch_* and of tu_fwd.hip / tu_bwd_block.inc /
    tu_bwdw.hip / tu_bwd_first.hip, restated:
    - "fwd_first" (shape = (K1, C1, CO, K, S)): the x6 first convolution ("conv1_x6_fwd") exists for stride 1 in fp32 mode; the
      bf16 modes ignore it.
    - "bwd_first": fp32 mode with "bwd_wide" tries the 512-thread bwd_firstw_kernel first - its x6 form for 3-tap stride-1 conv1
      under "conv1_x6" and "bwd_first_wide", its plain form for strides > 1, nothing for the rest; otherwise bwd_first_kernel,
      whose x6 conv1 weight gradient ("conv1_x6") exists for stride 1 in every mode.
    - "fwd_block" (shape = (CI, CO, K)): one form per mode.
    - "bwd_block": "bwd_wide" runs square 48- and 64-wide blocks as the 512-thread bwd_blockw_kernel (every mode), the rest as
      bwd_block_kernel; both have a LAST form for the model's last block."""
    o = dict(OPTION_DEFAULTS, **options)
    bf, sb = mode >= 1, mode == 2
    if kind == "fwd_first":
        k1, c1, co, k, s = shape
        x6 = mode == 0 and s == 1 and bool(o["conv1_x6_fwd"])
        return "fwd_first_kernel<%d, %d, %d, %d, %d, %s, %s, %s>" % (k1, c1, co, k, s, _b(bf), _b(sb), _b(x6))
    if kind == "bwd_first":
        k1, c1, co, k, s = shape
        if mode == 0 and o["bwd_wide"]:
            if o["conv1_x6"] and o["bwd_first_wide"] and s == 1 and k1 == 3 and co <= 64:
                return "bwd_firstw_kernel<%d, %d, %d, %d, %d, 512, true>" % (k1, c1, co, k, s)
            if s > 1:
                return "bwd_firstw_kernel<%d, %d, %d, %d, %d, 512, false>" % (k1, c1, co, k, s)
        x6 = s == 1 and bool(o["conv1_x6"])
        return "bwd_first_kernel<%d, %d, %d, %d, %d, %s, %s, %s>" % (k1, c1, co, k, s, _b(bf), _b(sb), _b(x6))
    if kind == "fwd_block":
        ci, co, k = shape
        return "fwd_block_kernel<%d, %d, %d, %s, %s>" % (ci, co, k, _b(bf), _b(sb))
    if kind == "bwd_block":
        ci, co, k = shape
        if o["bwd_wide"] and ci == co and ci in (48, 64):
            return "bwd_blockw_kernel<%d, %d, %d, %s, 512, %s, %s>" % (ci, co, k, _b(last), _b(bf), _b(sb))
        return "bwd_block_kernel<%d, %d, %d, %s, %s, %s>" % (ci, co, k, _b(last), _b(bf), _b(sb))
    raise ValueError(kind)


def _option_sets():
    names = sorted(OPTION_DEFAULTS)
    return [dict(zip(names, v)) for v in itertools.product((0, 1), repeat=len(names))]


def _modes_of(bf16):
    return (1, 2) if bf16 else (0,)


@functools.lru_cache(maxsize=None)
def _inventory(lib):
    """{instantiation: (launcher kind, shape, mode)} over the table, every mode its shapes have and every option set."""
    inv = {}
    for bf16, (firsts, blocks) in _tables(lib).items():
        for mode, o in itertools.product(_modes_of(bf16), _option_sets()):
            for f in firsts:
                for kind in ("fwd_first", "bwd_first"):
                    inv.setdefault(instantiation(kind, f, mode, o), (kind, f, mode))
            for b in blocks:
                inv.setdefault(instantiation("fwd_block", b, mode, o), ("fwd_block", b, mode))
                for last in (False, True):
                    inv.setdefault(instantiation("bwd_block", b, mode, o, last), ("bwd_block", b, mode))
    return inv


def inventory(lib):
    """Every kernel instantiation the library's launchers can reach: (table shape) x (every form its launcher can pick)."""
    return frozenset(_inventory(lib))


def launcher_of(inst):
    return inst.split("<")[0]


def first_stride(inst):
    """The conv1 stride of a first-block instantiation (template argument 5), None for a block kernel."""
    if not inst.startswith(("fwd_first", "bwd_first")):
        return None
    return int(inst.split("<")[1].split(",")[4])


def required(lib):
    """What the plan must cover: every instantiation, and every strided first-block instantiation once in tail mode and once
    over two or more 64-row tiles (("tail", inst), ("two-tile", inst))."""
    inv = inventory(lib)
    strided = [i for i in inv if (first_stride(i) or 1) > 1]
    return frozenset(inv) | {("tail", i) for i in strided} | {("two-tile", i) for i in strided}


# ------------------------------------------------------------------------------------------ plan
def tile_mode(first, T):
    """"tail" (a0 rows Ta in TT + 1 .. TT + K - 1 of a strided conv1: one tile whose rows behind the 64th ride along,
    fwd_first_body.inc), "two-tile" (more rows than that: two or more tiles) or "one" (Ta <= TT)."""
    k1, _, _, k, s = first
    ta = (T - k1) // s + 1
    if s > 1 and TT < ta <= TT + k - 1:
        return "tail"
    return "two-tile" if ta > TT else "one"


def case_kernels(case):
    """The instantiations a case launches, in launch order (forward, then backward)."""
    mode, o, first, blocks = case["mode"], case["options"], case["first"], case["blocks"]
    out = [instantiation("fwd_first", first, mode, o)] + [instantiation("fwd_block", b, mode, o) for b in blocks]
    out += [instantiation("bwd_block", b, mode, o, i == len(blocks) - 1) for i, b in reversed(list(enumerate(blocks)))]
    return out + [instantiation("bwd_first", first, mode, o)]


def case_items(case):
    """What a case covers (the terms of required())."""
    ks = set(case_kernels(case))
    tm = tile_mode(case["first"], case["T"])
    if case["first"][4] > 1 and tm != "one":
        ks |= {(tm, instantiation(kind, case["first"], case["mode"], case["options"])) for kind in ("fwd_first", "bwd_first")}
    return ks


def case_flags(case):
    """Model flags + engine options of a case (engine_checks.make_engine reads the options out of the flags)."""
    k1, c1, _, _, s = case["first"]
    widths = [case["first"][2]] + [b[1] for b in case["blocks"]]
    n = len(widths)
    flags = dict(mo.MIXEDNET_DEFAULTS, pointwise_filters=",".join(map(str, widths)), repeat_in_block=",".join(["1"] * n),
                 residual_connection=",".join(["0"] * n), mixconv_kernel_sizes=",".join(str(list(g)) for g in case["groups"]),
                 first_conv_filters=c1, first_conv_kernel_size=k1, stride=s)
    if case["mode"] == 1:
        flags["pw_bf16"] = True
    elif case["mode"] == 2:
        flags["st_bf16"] = True
    flags.update(case["options"])
    return flags


def _shape_tag(kind, shape):
    if kind.endswith("first"):
        k1, c1, co, k, s = shape
        return "f%dx%dx%dk%ds%d" % (k1, c1, co, k, s)
    ci, co, k = shape
    return "b%dx%dk%d" % (ci, co, k)


def _form_tag(inst):
    """"narrow" / "wide" / "x6" / "wide-x6" / "exact" of an instantiation (the id of a case names its anchor's form)."""
    args = inst.split("<")[1].rstrip(">").split(", ")
    name = launcher_of(inst)
    if name == "bwd_blockw_kernel":
        return "wide"
    if name == "bwd_block_kernel":
        return "narrow"
    if name == "bwd_firstw_kernel":
        return "wide-x6" if args[6] == "true" else "wide"
    if name == "bwd_first_kernel":
        return "narrow-x6" if args[7] == "true" else "narrow"
    if name == "fwd_first_kernel":
        return "x6" if args[7] == "true" else "exact"
    return "fwd"


class _Planner:
    def __init__(self, lib, seed):
        self.rng = random.Random(seed)
        tabs = _tables(lib)
        self.firsts = {m: tabs[m > 0][0] for m in MODES}
        self.blocks = {m: tabs[m > 0][1] for m in MODES}
        self.need = set(required(lib))
        self.cases = []
        # fewest blocks from pointwise width a to width b (0: a == b)
        self.hops = {}
        for m in MODES:
            ws = sorted({b[0] for b in self.blocks[m]} | {b[1] for b in self.blocks[m]})
            h = {(a, b): (0 if a == b else 99) for a in ws for b in ws}
            for ci, co, _ in self.blocks[m]:
                h[(ci, co)] = min(h[(ci, co)], 1)
            for k, a, b in itertools.product(ws, ws, ws):
                h[(a, b)] = min(h[(a, b)], h[(a, k)] + h[(k, b)])
            self.hops[m] = h

    def gain(self, items):
        return sum(1 for i in items if i in self.need)

    @staticmethod
    def _ta_max(first, tm):
        """most a0 rows a case of tile mode tm may have (stride 1: none but keeping T small)"""
        return {"tail": TT + first[3] - 1, "two-tile": TT + first[3] + 40, "one": TT if first[4] > 1 else 160}[tm]

    def _ta(self, first, tm, used, final):
        """a0 rows for tile mode tm with `used` rows eaten by the depthwise convolutions and >= `final` final frames left."""
        lo = max({"tail": TT + 1, "two-tile": TT + first[3], "one": 1}[tm], used + final)
        hi = self._ta_max(first, tm)
        if lo > hi:
            return None
        if tm == "one":
            return lo + self.rng.randrange(0, min(8, hi - lo + 1))   # T stays small
        return self.rng.randint(lo, hi)

    def build(self, mode, last=None, middle=None, wide=None, first_must=None):
        """One case of `mode` ending in block `last` (None: chosen), holding block `middle` right behind the first block if
        given, "bwd_wide" = `wide` if given; the first block, its options and tile mode chosen for the most uncovered items."""
        rng = self.rng
        opt_sets = [o for o in _option_sets() if wide is None or o["bwd_wide"] == wide]
        best, best_key = None, None
        for first in self.firsts[mode]:
            co = first[2]
            if middle is not None and co != middle[0]:
                continue
            w_after = middle[1] if middle is not None else co
            slots = MAX_BLOCKS[mode > 0] - 2 - (middle is not None)
            if last is not None and self.hops[mode].get((w_after, last[0]), 99) > slots:
                continue
            # a0 rows the fixed blocks need at least (a 3-tap block per width hop, 3 taps for a last block still to choose)
            fixed = (first[3] - 1 + (last[2] - 1 if last is not None else 2) + (middle[2] - 1 if middle is not None else 0)
                     + 2 * (self.hops[mode][(w_after, last[0])] if last is not None else 0) + MIN_FINAL_FRAMES[mode > 0])
            for o in opt_sets:
                kf, kb = instantiation("fwd_first", first, mode, o), instantiation("bwd_first", first, mode, o)
                for tm in (("tail", "two-tile", "one") if first[4] > 1 else ("one",)):
                    if fixed > self._ta_max(first, tm):
                        continue
                    items = [kf, kb] + ([(tm, kf), (tm, kb)] if tm != "one" else [])
                    if first_must is not None and first_must not in items:
                        continue
                    if last is not None:
                        items.append(instantiation("bwd_block", last, mode, o, True))
                    if middle is not None:
                        items.append(instantiation("bwd_block", middle, mode, o, False))
                    key = (self.gain(items), tm == "one", first[4] == 1, rng.random())
                    if best_key is None or key > best_key:
                        best, best_key = (first, o, tm), key
        if best is None:
            raise RuntimeError("no first block for mode %d last %s middle %s" % (mode, last, middle))
        first, o, tm = best
        final = MIN_FINAL_FRAMES[mode > 0]
        budget = self._ta_max(first, tm) - final   # a0 rows the depthwise convolutions may eat
        budget -= first[3] - 1
        blocks = [middle] if middle is not None else []
        budget -= sum(b[2] - 1 for b in blocks)
        w = blocks[-1][1] if blocks else first[2]
        reserve = (last[2] - 1) if last is not None else 2
        # middle blocks: the most uncovered items first; none once nothing new is left, unless the widths need a bridge
        while len(blocks) < MAX_BLOCKS[mode > 0] - 2:
            target = last[0] if last is not None else None
            room = MAX_BLOCKS[mode > 0] - 2 - len(blocks) - 1   # slots left after this one
            cands = []
            for b in self.blocks[mode]:
                if b[0] != w or b[2] - 1 > budget - reserve:
                    continue
                if target is not None and (self.hops[mode].get((b[1], target), 99) > room
                                           or b[2] - 1 + 2 * self.hops[mode][(b[1], target)] > budget - reserve):
                    continue   # (a bridge back to the last block's width costs at least a 3-tap block per hop)
                items = [instantiation("fwd_block", b, mode, o), instantiation("bwd_block", b, mode, o, False)]
                cands.append((self.gain(items), rng.random(), b))
            if not cands:
                break
            g, _, b = max(cands)
            bridge = target is not None and w != target
            if g == 0 and not bridge:
                break
            blocks.append(b)
            budget -= b[2] - 1
            w = b[1]
        if last is None:
            cands = [(self.gain([instantiation("bwd_block", b, mode, o, True), instantiation("fwd_block", b, mode, o)]), rng.random(), b)
                     for b in self.blocks[mode] if b[0] == w and b[2] - 1 <= budget]
            last = max(cands)[2]
        assert last[0] == w, (first, blocks, last)
        blocks.append(last)
        used = (first[3] - 1) + sum(b[2] - 1 for b in blocks)
        ta = self._ta(first, tm, used, final)
        assert ta is not None, (first, tm, blocks)
        T = (ta - 1) * first[4] + first[0] + rng.randrange(first[4])   # frames past the last stride step are never read
        # MixConv groups now and then (the kernel runs them fused to the longest: zero taps + gradient mask)
        groups = []
        for k in [first[3]] + [b[2] for b in blocks]:
            if k > 3 and rng.random() < 0.25:
                groups.append(sorted(rng.sample(range(1, k, 2), min(2, (k - 1) // 2))) + [k])
            else:
                groups.append([k])
        case = dict(mode=mode, options=o, first=first, blocks=tuple(blocks), groups=groups, T=T,
                    B=rng.randint(8 if mode > 0 else min(8, -(-MIN_BN_ROWS // (ta - used))), 8), grid=rng.choice([1, 2, 3, 5, 8, 0]))
        assert first[4] == 1 or tile_mode(first, T) == tm, (first, T, tm)
        self.need -= case_items(case)
        self.cases.append(case)
        return case


@functools.lru_cache(maxsize=None)
def _plan(lib, seed):
    p = _Planner(lib, seed)
    # 1. one case per LAST backward instantiation (only a model's last block runs it)
    lasts = {}
    for m in MODES:
        for b in p.blocks[m]:
            for wide in (0, 1):
                inst = instantiation("bwd_block", b, m, dict(bwd_wide=wide), True)
                lasts[inst] = (m, b, None) if inst in lasts else (m, b, wide)   # None: the same kernel either way
    order = sorted(lasts)
    p.rng.shuffle(order)
    for inst in order:
        m, b, wide = lasts[inst]
        c = p.build(m, last=b, wide=wide)
        c["id"] = "%s-last-%s-%s" % (_shape_tag("block", b), _form_tag(inst), MODE_NAME[m])
    # 2. first-block instantiations and tile modes still open
    meta = _inventory(lib)
    for item in sorted(p.need, key=str):
        inst = item[1] if isinstance(item, tuple) else item
        kind, shape, m = meta[inst]
        if item not in p.need or kind not in ("fwd_first", "bwd_first"):
            continue
        c = p.build(m, first_must=item)
        c["id"] = "%s-%s-%s-%s-%s" % (_shape_tag(kind, shape), kind.replace("_first", ""), _form_tag(inst),
                                      tile_mode(c["first"], c["T"]), MODE_NAME[m])
    # 3. block instantiations not yet run (as a middle block: the LAST forms are all run by step 1)
    for item in sorted(p.need, key=str):
        if item not in p.need:
            continue
        kind, shape, m = meta[item]
        wide = (1 if item.startswith("bwd_blockw") else 0) if kind == "bwd_block" else None
        c = p.build(m, middle=shape, wide=wide)
        c["id"] = "%s-%s-%s" % (_shape_tag(kind, shape), _form_tag(item), MODE_NAME[m])
    seen = {}
    for c in p.cases:
        n = seen.get(c["id"], 0)
        seen[c["id"]] = n + 1
        if n:
            c["id"] += "-%d" % n
    return tuple(p.cases), frozenset(p.need)


def plan(lib, seed=2026):
    """The sweep: a list of cases, each a dict with the model (first block shape, block shapes, MixConv groups), the mode and
    engine options, T, B, grid and an id naming its anchor instantiation (e.g. ``b48x64k21-last-narrow-fp32``)."""
    return list(_plan(lib, seed)[0])


def uncovered(lib, seed=2026):
    """Items of required() that plan() does not cover (empty when the plan is complete)."""
    cov = set()
    for c in plan(lib, seed):
        cov |= case_items(c)
    return sorted(set(required(lib)) - cov, key=str)


def describe(case):
    return "%s: mode %s options %s conv1 %d/%d stride %d, first dw %d, blocks %s, kernels %s, T %d (%s) B %d grid %d" % (
        case["id"], MODE_NAME[case["mode"]], case["options"], case["first"][0], case["first"][1], case["first"][4],
        case["first"][3], list(case["blocks"]), case["groups"], case["T"], tile_mode(case["first"], case["T"]), case["B"], case["grid"])


def form_of(inst):
    """An instantiation without its shape: launcher + the form arguments (LAST, threads, bf16 operands / storage, x6)."""
    name, args = inst.rstrip(">").split("<")
    n_shape = 5 if "first" in name else 3
    return "%s<%s>" % (name, ", ".join(args.split(", ")[n_shape:]))


def case_forms(case):
    forms = {form_of(i) for i in case_kernels(case)}
    tm = tile_mode(case["first"], case["T"])
    if case["first"][4] > 1 and tm == "tail":
        forms.add("tail: " + form_of(instantiation("bwd_first", case["first"], case["mode"], case["options"])))
    return forms


def emulator_slice(lib, seed=2026):
    """A fixed slice of the plan for the emulated kernels (tests/hipemu): every form (case_forms: launcher x LAST / narrow / wide
    / fp32 / bf16 / bf16st / x6 / exact, and each first-block backward form in tail mode) and every table shape at least once,
    greedily, cheapest case first among equals."""
    cases = plan(lib, seed)

    def items(c):
        return case_forms(c) | {("first", c["first"])} | {("block", b) for b in c["blocks"]}

    cost = {c["id"]: c["B"] * c["T"] * (len(c["blocks"]) + 1) for c in cases}
    todo = set().union(*(items(c) for c in cases))
    out = []
    while todo:
        best = max(cases, key=lambda c: (len(items(c) & todo), -cost[c["id"]]))
        out.append(best)
        todo -= items(best)
    return out
