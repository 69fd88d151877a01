"""A covering sweep of the two run-time-shape streaming kernels - ``stream_forward_kernel<false, *>`` (csrc/tu_stream.hip, with its
calibration form ``<REC = true>``) and ``stream_q8_kernel<false>`` (csrc/tu_stream_q8.hip), the forms a plain MixedNet runs - shared by the GPU sweep
(tests/test_stream_sweep_gpu.py) and its CPU-side checks (tests/test_stream_sweep_emulated.py).

``plan()`` in csrc/stream_common.hip.h accepts far more than the topologies the realistic tests run (widths that are no
multiple of 4, uneven MixConv splits, blocks without a depthwise layer, k1 <= stride, t_final = 1, 128 layers, tiles on
either side of the LDS limit).  So:

- ``cases()`` is a deterministic, seeded (SEED) list of small cases.  A case is a stream description built directly (run
  through ``native.Stream`` in the context of any float model), Keras-order weights for it (``OracleModel`` +
  ``engine_checks.perturbed_oracle`` of the equivalent flag set, BatchNorm statistics taken from a float64 dry run as
  training would leave them), a call script, and an id that names what it was built around.  The cases are written by hand;
  what each one covers is COMPUTED from its description, its script and an oracle dry run (``items_of``), not claimed.
- ``required()`` lists the items the plan must cover; ``uncovered()`` must come back empty.
- ``run_case(lib, case)`` drives one case through the float kernel, its REC form and the int8 kernel and holds every call
  to the float64 / integer oracles (tests/streaming_oracle.py, tests/quant_oracle.py): outputs, logits AND rings.
- two conditions on a case's INPUTS are checked from the oracles alone (``float32_condition``, ``q8_checks.check_spread``):
  the float32 restatement of the oracle stays within a quarter of each bound of the float64 one, and the int8 logits the
  comparison sees are spread out (a comparison of a near-constant passes whatever the kernel computes).
"""
import functools
import time

import numpy as np

import engine_checks as ec
import q8_checks as qc
import quant_oracle as qo
import streaming_checks as sc
import streaming_oracle as so

SEED = 2026
KMAX_LDS = 160 * 1024   # kMaxLds of csrc/stream_common.hip.h
TILE = 256              # kTileOutputs of csrc/stream_common.hip.h
CHAIN_MAX_RING = 40     # one-output chains run where the longest ring is at most this (they cost one call per output)


# ------------------------------------------------------------------------------------------------- descriptions
def desc_of(c1, k1, s, blocks, tf, frames=None):
    d = dict(conv1_filters=c1, conv1_kernel=k1, stride=s, blocks=[(r, tuple(ks), f) for r, ks, f in blocks], t_final=tf,
             frames=0, mode="stream")
    d["frames"] = sc.frames_of(d) if frames is None else frames
    return d


def layers_of(desc):
    """[(kind, K or None, cin, cout, kernel sizes)] in plan order, as csrc/stream_common.hip.h plan() lays them out"""
    out, c = [], desc["conv1_filters"]
    for rep, ks, f in desc["blocks"]:
        for _ in range(rep):
            if max(ks) > 1:
                out.append(("mix", max(ks), c, c, ks))
            out.append(("pw", None, c, f, ks))
            c = f
    return out


def reach1_of(desc):
    return desc["t_final"] - 1 + sum(k - 1 for kind, k, _, _, _ in layers_of(desc) if kind == "mix")


def cmax_of(desc):
    return max([desc["conv1_filters"]] + [co for _, _, _, co, _ in layers_of(desc)])


def r4(n):
    return (n + 3) & ~3


def tile_bytes(desc):
    """bytes of one int8 tile (MixedNet::plan restated): the gathered input rows and two activation buffers"""
    rows = TILE + reach1_of(desc)
    return ((rows - 1) * desc["stride"] + desc["conv1_kernel"]) * 40 + 2 * rows * r4(cmax_of(desc))


def tile_placement(desc):
    b = tile_bytes(desc)
    if b > KMAX_LDS:
        return "scratch"
    return "lds<64K" if b <= 64 * 1024 else "lds-64K-160K"


def ring_lengths(desc):
    return ([max(0, desc["conv1_kernel"] - desc["stride"])] + [k - 1 for kind, k, _, _, _ in layers_of(desc) if kind == "mix"]
            + [desc["t_final"] - 1])


# ------------------------------------------------------------------------------------------------------- cases
class Case:
    """``script``: stream-mode steps run in order on one stream -
         ("tracks", lengths, pads)   one mww_stream_run over resident tracks (even tracks u16, odd f32)
         ("host", n_frames)          one mww_stream_run_host
         ("outputs", n)              a host call of exactly n outputs; n = "grid": more tiles than 2 x CU workgroups
         ("ones", n)                 n successive one-output host calls (the oracle is the literal StepStream while every
                                     call since the reset was one)
         ("zero",)                   a host call of fewer than ``stride`` frames: no output, state untouched
         ("reset",)
       ``ns``: (lengths, pads) of the non-stream twin (description ``frames`` = the window).  ``two`` runs a second stream
       of the same context alternately.  ``w_edit`` / ``r_edit`` / ``i_edit`` are the hand edits of the dedicated
       requantization cases: float weights before anything is derived from them, calibrated ranges, int32 values."""

    def __init__(self, cid, desc, script=None, ns=None, two=False, w_edit=None, r_edit=None, i_edit=None, spread=True, cap=1200, bn_shift=0.0, dense_scale=1.0):
        self.id, self.desc, self.two = cid, desc, two
        s, T = desc["stride"], desc["frames"]
        chain = max(ring_lengths(desc)) + 2
        self.script = script if script is not None else [
            ("tracks", [0, 7, T + 5, 0, 3, 2 * T + s + 1, 0], [0, 2, 0, 0, 0, 4, 0]),
            ("zero",),
            ("host", T + 9),
            ("reset",),
            ("ones", chain if chain - 2 <= CHAIN_MAX_RING else 3),
            ("tracks", [300 * s + 1, 2], [0, 0]),
        ]
        self.ns = ns if ns is not None else ([T, T - 1, 0, T + s - 1, T + 3 * s + 1], [T // 2, 0, 0, 0, 0])
        self.w_edit, self.r_edit, self.i_edit, self.spread = w_edit, r_edit, i_edit, spread
        # scalings of the random weights that keep the float32 restatement within a quarter of the bounds (float32_condition):
        # BatchNorm offsets in standard deviations, a factor on the Dense kernel and bias
        self.bn_shift, self.dense_scale = bn_shift, dense_scale
        self.cap = cap   # outputs of the sequence the chunking / REC / calibration checks run on
        assert spread == ("nospread" not in cid)   # a case that cannot reach the spread condition says so in its id

    def __repr__(self):
        return self.id


def _zero_and_tiny_channels(w, names):
    """float-weight edit: one all-zero pointwise output channel (weight scale 1) and one with tiny weights (an effective
    multiplier below 2^-16: right shifts >= 16)"""
    i = names.index("b0.r0.pw.kernel")
    w[i] = w[i].copy()
    w[i][..., 1] = 0.0
    w[i][..., 2] *= 1e-5
    return w


def _unnormalised_multipliers(qm):
    """int32 edit: the same effective multipliers written with a LEFT shift (M >> k, shift + k: the device takes any
    M >= 0), and the two shift edges on one channel each"""
    op = qm.ops[2]   # the first pointwise layer behind conv1 and one MixConv
    assert op["kind"] == "pw" and op["multiplier"].size >= 8
    for c in (0, 3, 4):
        k = 2 - int(op["shift"][c])
        assert 0 < k < 20
        op["multiplier"][c] >>= k
        op["shift"][c] += k
    op["shift"][5], op["shift"][6] = -31, 30
    d = qm.ops[-1]   # the Dense too: a left shift on the logit's own requantization
    k = 1 - int(d["shift"][0])
    assert 0 < k < 20
    d["multiplier"][0] >>= k
    d["shift"][0] += k


def cases():
    """the plan: small cases, each built around the axes its id names"""
    out = []
    # the two odd topologies of the issue: widths 30 / 50 / 7, three / two / one MixConv groups with a remainder split and
    # a group list that starts with kernel 1, k1 < stride; the window of the non-stream twin has (T - k1) % s != 0
    d = desc_of(13, 2, 3, [(1, (3, 5, 9), 30), (1, (1, 5), 50), (1, (3,), 7)], 4)
    out.append(Case("w30-50-7_g3-rem_k1lt-s3", dict(d, frames=d["frames"] + 1)))
    # widths 13 / 9, no depthwise layer in the first block, equal neighbouring kernels, k1 == stride, t_final = 1
    out.append(Case("w13-9_g3-eq_k1eq-s3_tf1", desc_of(7, 3, 3, [(1, (1,), 13), (1, (3, 3, 7), 9)], 1)))
    # conv1 is the widest layer; repeat 2; a middle block without a depthwise layer; stride 2 with a conv1 ring of 3 rows
    out.append(Case("cmax-first_rep2_k1-middle_s2", desc_of(36, 5, 2, [(2, (3,), 12), (1, (1,), 16), (1, (3, 5), 6)], 3), two=True))
    # stride 4, the last block without a depthwise layer, one-block neighbour below
    out.append(Case("s4_k1-last", desc_of(8, 6, 4, [(1, (3,), 10), (1, (1,), 5)], 2)))
    out.append(Case("one-block_s1", desc_of(5, 3, 1, [(1, (3, 5), 11)], 3)))
    # eight blocks; eight groups; a width-1 bottleneck
    out.append(Case("blocks8_g8_w1", desc_of(16, 3, 1, [(1, (1, 2, 3, 4, 5, 6, 7, 8), 16), (1, (3,), 1), (1, (3,), 9), (1, (2, 5), 11),
                                                        (1, (3,), 3), (1, (1,), 6), (1, (5,), 2), (1, (3,), 4)], 2),
                    dense_scale=0.5))   # (float32 restatement at 0.30 of PROB_TOL with the Dense scale at 1)
    # the deepest model the header allows: 8 x 8 repeats with depthwise layers = 128 layers, 131 tensors (= kMaxTensors),
    # and a halo (reach1 = 257) larger than one 256-output tile.  64 ReLU blocks of O(1) random weights are chaotic: with
    # the BatchNorm offsets at zero the float32 restatement of the ORACLE is 300 x FWD_TOL from the float64 one (the error
    # doubles every 8 layers).  Offsets of two standard deviations keep most units on the linear side and half the Dense
    # scale brings the probabilities within a quarter of PROB_TOL; the bounds stay as they are.
    out.append(Case("layers128_reach257", desc_of(4, 3, 1, [(8, (5,), f) for f in (5, 6, 4, 7, 5, 6, 4, 3)], 2),
                    script=[("tracks", [0, 40, 300, 0], [0, 3, 0, 0]), ("zero",), ("host", 530), ("reset",), ("ones", 6),
                            ("outputs", 257)], cap=700, bn_shift=2.0, dense_scale=0.5))
    # the widest pointwise layer plan() accepts (short calls)
    out.append(Case("w1024", desc_of(8, 3, 1, [(1, (3,), 1024), (1, (3,), 4)], 3),
                    script=[("tracks", [0, 60, 7, 0], [0, 2, 0, 0]), ("zero",), ("host", 70), ("reset",), ("ones", 5), ("outputs", 300)],
                    cap=330))
    # a head over more frames than a tile has outputs (head ring longer than a tile, halo larger than a tile)
    out.append(Case("tf300", desc_of(8, 3, 1, [(1, (3,), 8)], 300),
                    script=[("tracks", [0, 100, 320, 0], [0, 5, 0, 0]), ("zero",), ("outputs", 257), ("outputs", 513), ("reset",),
                            ("ones", 4), ("outputs", 330)], cap=900))
    # int8 tile placement: 64..160 KB; the largest tile that fits 160 KB (k1 = 3, s = 1, reach1 = 8: cmax = 288 gives
    # 162 704 B) and the smallest that does not (cmax = 292: 164 816 B)
    out.append(Case("lds-mid_w200", desc_of(8, 3, 1, [(1, (5,), 200), (1, (1,), 12)], 5), cap=600))
    out.append(Case("lds-largest_w288", desc_of(6, 3, 1, [(1, (3, 5), 288)], 5), cap=600))
    out.append(Case("scratch-smallest_w292", desc_of(6, 3, 1, [(1, (3, 5), 292), (1, (1,), 10)], 5), cap=600))
    # exact tile boundaries and more tiles than 2 x CU workgroups (the grid-stride loop), tiny widths
    out.append(Case("grid-stride_tile-edges", desc_of(4, 3, 1, [(1, (3,), 4)], 2),
                    script=[("outputs", 255), ("outputs", 256), ("zero",), ("outputs", 257), ("outputs", 513), ("outputs", "grid"),
                            ("reset",), ("ones", 5), ("outputs", 256)],
                    ns=([11, 7, 9, 0, 262 + 7], [0, 0, 2, 0, 0])))
    # the dedicated requantization cases: ranges and int32 values edited by hand (the oracle follows whatever they say)
    base = desc_of(8, 3, 1, [(1, (3,), 8), (1, (5,), 8)], 3)
    out.append(Case("rq-ranges", base, w_edit=_zero_and_tiny_channels,
                    r_edit={0: ("set", 5.0, 30.0),      # the input saturates at both ends
                            2: ("scale", 0.4),          # a MixConv output clamps at -128 and at 127
                            3: ("scale", 0.6),          # a ReLU output clamps at 127
                            4: ("sym",),                # zero point 0
                            }))
    out.append(Case("rq-shifts", base, i_edit=_unnormalised_multipliers,
                    r_edit={2: ("neg",),                # a MixConv output whose range ends at 0: zero point 127
                            4: ("set", 0.0, 0.0),       # a tensor of range (0, 0): scale 1, zero point 0
                            }))
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    cs = cases()
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


def case_ids():
    return [c.id for c in _cases()]


def case(cid):
    return next(c for c in _cases() if c.id == cid)


# ------------------------------------------------------------------------------------------- weights and frames
def _rng(cid, *extra):
    return np.random.default_rng([SEED] + [ord(ch) for ch in cid] + [int(e) for e in extra])


def gen_frames(rng, n, kind="f32"):
    """rows shaped like the features: u16-scaled values or float32 values"""
    if kind == "u16":
        return rng.integers(0, 1200, size=(n, 40)).astype(np.float32) * np.float32(0.0390625)
    return rng.uniform(0, 40, size=(n, 40)).astype(np.float32)


class Built:
    """everything derived from a case without a kernel: flags, the oracle model with its conditioned weights, the float64
    net, the sequence the chunking / REC checks run on, the int8 model and what the oracles say about the inputs"""


def _condition_bn(flags, om, frames, shift=0.0):
    """BatchNorm moving statistics := the statistics of each 1x1 layer's output on a float64 dry run (what training
    leaves there): every layer's activations stay of order one however deep or wide the model is"""
    names = [v.name for v in om.vars]
    w = om.get_weights()
    for _ in range(1):
        net = so.Net(flags, om)
        x = np.concatenate([np.zeros((net.r1, 40)), np.asarray(frames, np.float64)], 0)
        a = net.conv1(x)
        for kind, p, ks in net.layers:
            if kind == "mix":
                a = net.mix(p, ks, np.concatenate([np.zeros((max(ks) - 1, a.shape[1])), a], 0))
            else:
                y = a @ net.w[p + ".pw.kernel"][0, 0]
                var = y.var(axis=0)
                w[names.index(p + ".bn.moving_mean")] = (y.mean(axis=0) - shift * np.sqrt(var)).astype(np.float32)
                w[names.index(p + ".bn.moving_variance")] = np.where(var > 1e-12, var, 1.0).astype(np.float32)
                om.set_weights(w)
                net = so.Net(flags, om)
                a = net.pw(p, a)
    return om


@functools.lru_cache(maxsize=None)
def built(cid):
    c = case(cid)
    b = Built()
    b.case, b.desc = c, c.desc
    b.flags = sc.flags_of(c.desc)
    b.T, b.s = c.desc["frames"], c.desc["stride"]
    om = ec.perturbed_oracle(b.T, seed=SEED, flags=b.flags)
    assert so.Net(b.flags, om).tf == c.desc["t_final"], (cid, so.Net(b.flags, om).tf)
    if c.dense_scale != 1.0:
        om.set_weights([w * np.float32(c.dense_scale) if v.name.startswith("dense.") else w for v, w in zip(om.vars, om.get_weights())])
    if c.w_edit:
        om.set_weights(c.w_edit(om.get_weights(), [v.name for v in om.vars]))
    b.seq = gen_frames(_rng(cid, 0), c.cap * b.s, "u16")
    b.seq[0, 0], b.seq[0, 1] = 0.0, 26.0
    if c.r_edit and 0 in c.r_edit:   # a case that narrows the input range also feeds rows below zero (saturation at -128)
        b.seq[5:50] -= np.float32(8.0)
    b.om = _condition_bn(b.flags, om, b.seq, c.bn_shift)
    b.net = so.Net(b.flags, b.om)
    b.weights = b.om.get_weights()
    b.flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in b.weights])
    # the int8 model: ranges from the float64 dry run of the same weights, then the case's hand edits
    ranges = qc.float64_ranges(b.om, b.flags, b.seq)
    for t, e in (c.r_edit or {}).items():
        lo, hi = ranges[t]
        ranges[t] = {"set": lambda: (e[1], e[2]), "scale": lambda: (lo * e[1], hi * e[1]), "sym": lambda: (-max(-lo, hi), max(-lo, hi)),
                     "neg": lambda: (lo, 0.0)}[e[0]]()
    from microwakeword_amd import quantize
    b.qm = quantize.quantize_weights(c.desc, b.weights, ranges.astype(np.float32))
    if c.i_edit:
        c.i_edit(b.qm)
    return b


def float32_condition(cid):
    """the float32 restatement against the float64 one over the case's sequence, as fractions of the bounds:
    (logits / FWD_TOL, probabilities / PROB_TOL, activation rings / FWD_TOL).  The plan's CPU test asserts each <= 1/4."""
    b = built(cid)
    z64, st64 = so.whole_sequence(b.net, b.seq, rings=True)
    z32, st32 = so.whole_sequence(so.Net(b.flags, b.om, dtype=np.float32), b.seq, rings=True)
    n1 = b.net.r1 * 40
    return (float(np.abs(z32 - z64).max()) / ec.FWD_TOL, float(np.abs(so.sigmoid(z32) - so.sigmoid(z64)).max()) / sc.PROB_TOL,
            (float(np.abs(st32[n1:] - st64[n1:]).max()) if st64.size > n1 else 0.0) / ec.FWD_TOL)


@functools.lru_cache(maxsize=None)
def oracle_report(cid):
    """what the int8 oracle does on the case's sequence: (spread triple, branches taken) - both from the oracle alone"""
    b = built(cid)
    with qo.record_branches() as seen:
        sp = qc.spread(b.qm, b.seq)
        seen = set(seen)
    for op in b.qm.ops:
        w = op["weights"].astype(np.int64).reshape(-1, op["weight_scales"].size) if op["kind"] != "dense" else op["weights"].reshape(-1, 1)
        if np.any((np.abs(w).max(axis=0) == 0) & (op["weight_scales"] == 1)):
            seen.add("zero-weight-channel")
    if np.any((b.qm.ranges[:, 0] == 0) & (b.qm.ranges[:, 1] == 0)):
        seen.add("range-0-0")
    return sp, frozenset(seen)


# ------------------------------------------------------------------------------------------------------- items
BRANCH_ITEMS = ("rq-left-shift", "rq-right-shift>=16", "rq-clamp-low-relu", "rq-clamp-low-norelu", "rq-clamp-127", "rq-zp-out=-128",
                "rq-zp-out=0", "rq-zp-out=127", "in-sat-low", "in-sat-high", "zero-weight-channel", "range-0-0", "rq-shift=-31",
                "rq-shift=+30")


def required():
    it = ["conv1:k1>s", "conv1:k1==s", "conv1:k1<s"] + ["conv1:s=%d" % s for s in (1, 2, 3, 4)] + ["conv1:c1%%4=%d" % r for r in range(4)]
    it += ["depth:blocks=1", "depth:blocks=8", "depth:repeat=1", "depth:repeat=2", "depth:repeat=8", "depth:layers=128"]
    it += ["mix:groups=%d" % g for g in (1, 2, 3, 8)] + ["mix:split-remainder", "mix:starts-with-k1", "mix:equal-neighbours",
                                                          "mix:K1-first-block", "mix:K1-middle-block", "mix:K1-last-block"]
    it += ["width:pw-Ci%%4=%d" % r for r in (1, 2, 3)] + ["width:pw-Co%%4=%d" % r for r in (1, 2, 3)]
    it += ["width:c_last%4!=0", "width:1", "width:1024", "width:cmax-first", "width:cmax-middle", "width:cmax-last", "width:widening-pair",
           "width:narrowing-pair"]
    it += ["head:tf=1", "head:tf>256", "head:reach1>256"]
    it += ["tile:lds<64K", "tile:lds-64K-160K", "tile:lds-largest", "tile:scratch-smallest"]
    it += ["call:outputs=%d" % n for n in (255, 256, 257, 513)]
    it += ["call:one-output-chain", "call:zero-output-between", "call:empty-track-first", "call:empty-track-middle", "call:empty-track-last",
           "call:padded-tracks", "call:frames-u16", "call:frames-f32", "call:frames-host", "call:reset-between", "call:two-streams",
           "call:tiles>2CU"]
    it += ["ns:(T-k1)%s!=0", "ns:track=T", "ns:track=T-1", "ns:track=T+s-1", "ns:>256-windows-behind-short"]
    return it + list(BRANCH_ITEMS)


def items_of(c, with_oracle=True):
    """the items a case covers, computed from its description, its script and (the requantization branches) the oracle"""
    d = c.desc
    k1, s, c1, tf = d["conv1_kernel"], d["stride"], d["conv1_filters"], d["t_final"]
    it = {"conv1:k1>s" if k1 > s else ("conv1:k1==s" if k1 == s else "conv1:k1<s"), "conv1:s=%d" % s, "conv1:c1%%4=%d" % (c1 % 4)}
    nb = len(d["blocks"])
    it.add("depth:blocks=%d" % nb)
    L = layers_of(d)
    if len(L) == 128:
        it.add("depth:layers=128")
    cin = c1
    for bi, (rep, ks, f) in enumerate(d["blocks"]):
        it.add("depth:repeat=%d" % rep)
        if max(ks) > 1:
            it.add("mix:groups=%d" % len(ks))
            if cin % len(ks):
                it.add("mix:split-remainder")
            if ks[0] == 1 and len(ks) > 1:
                it.add("mix:starts-with-k1")
            if any(a == b for a, b in zip(ks, ks[1:])):
                it.add("mix:equal-neighbours")
        elif nb > 1:
            it.add("mix:K1-first-block" if bi == 0 else ("mix:K1-last-block" if bi == nb - 1 else "mix:K1-middle-block"))
        cin = f
    widths = [c1] + [co for kind, _, _, co, _ in L if kind == "pw"]
    for kind, _, ci, co, _ in L:
        if kind == "pw":
            if ci % 4:
                it.add("width:pw-Ci%%4=%d" % (ci % 4))
            if co % 4:
                it.add("width:pw-Co%%4=%d" % (co % 4))
            if co > ci:
                it.add("width:widening-pair")
            if co < ci:
                it.add("width:narrowing-pair")
            if co in (1, 1024):
                it.add("width:%d" % co)
    cm, c_last = max(widths), widths[-1]
    if c_last % 4:
        it.add("width:c_last%4!=0")
    if widths.count(cm) == 1 and len(widths) > 2:
        # cmax set by the first layer (conv1) or a middle one with c_last != cmax; set by the last layer it IS c_last, and
        # then every earlier row is narrower than the pitch (the item asks for a last layer that alone sets the pitch)
        at = widths.index(cm)
        it.add("width:cmax-first" if at == 0 else ("width:cmax-last" if at == len(widths) - 1 else "width:cmax-middle"))
    elif widths.count(cm) == 1 and len(widths) == 2:
        it.add("width:cmax-first" if widths[0] == cm else "width:cmax-last")
    if tf == 1:
        it.add("head:tf=1")
    if tf > TILE:
        it.add("head:tf>256")
    if reach1_of(d) > TILE:
        it.add("head:reach1>256")
    if tile_placement(d) != "scratch":
        it.add("tile:" + tile_placement(d))
    # the two tiles next to the limit: one more / one fewer pitch step of 4 channels changes the placement
    step = 2 * (TILE + reach1_of(d)) * 4
    if tile_bytes(d) <= KMAX_LDS < tile_bytes(d) + step:
        it.add("tile:lds-largest")
    if tile_bytes(d) - step <= KMAX_LDS < tile_bytes(d):
        it.add("tile:scratch-smallest")
    # stream-mode script
    since_reset_ones, n_calls = True, 0
    for i, st in enumerate(c.script):
        if st[0] == "tracks":
            lens, pads = st[1], st[2]
            it.update({"call:frames-u16"} | ({"call:frames-f32"} if len(lens) > 1 else set()))
            if lens[0] == 0:
                it.add("call:empty-track-first")
            if lens[-1] == 0:
                it.add("call:empty-track-last")
            if any(v == 0 for v in lens[1:-1]):
                it.add("call:empty-track-middle")
            if any(pads):
                it.add("call:padded-tracks")
        if st[0] in ("host", "outputs", "ones"):
            it.add("call:frames-host")
        if st[0] == "outputs":
            if st[1] == "grid":
                it.add("call:tiles>2CU")
            elif st[1] in (255, 256, 257, 513):
                it.add("call:outputs=%d" % st[1])
        if st[0] == "ones":
            if since_reset_ones and st[1] >= max(ring_lengths(d)) + 2:
                it.add("call:one-output-chain")
        elif st[0] == "reset":
            since_reset_ones = True
            if 0 < i < len(c.script) - 1:
                it.add("call:reset-between")
        elif st[0] != "zero":
            since_reset_ones = False
        if st[0] == "zero" and 0 < i < len(c.script) - 1 and c.script[i - 1][0] != "reset" and c.script[i + 1][0] != "reset":
            it.add("call:zero-output-between")
    if c.two:
        it.add("call:two-streams")
    # non-stream twin
    T = d["frames"]
    if (T - k1) % s:
        it.add("ns:(T-k1)%s!=0")
    lens = c.ns[0]
    for name, v in (("ns:track=T", T), ("ns:track=T-1", T - 1), ("ns:track=T+s-1", T + s - 1)):
        if v in lens:
            it.add(name)
    if lens and (lens[-1] - T) // s + 1 > TILE and len(lens) > 2:
        it.add("ns:>256-windows-behind-short")
    if with_oracle:
        it |= set(oracle_report(c.id)[1]) & set(BRANCH_ITEMS)
    return it


def uncovered(case_list=None):
    have = set()
    for c in (case_list if case_list is not None else _cases()):
        have |= items_of(c)
    return [i for i in required() if i not in have]


def describe(c):
    d = c.desc
    return "%s: conv1 %d x k%d s%d, blocks %s, t_final %d, window %d, reach1 %d, int8 tile %d B (%s), items %s" % (
        c.id, d["conv1_filters"], d["conv1_kernel"], d["stride"], d["blocks"], d["t_final"], d["frames"], reach1_of(d), tile_bytes(d),
        tile_placement(d), sorted(items_of(c, with_oracle=False)))


def cost(c):
    """a rough count of multiply-adds of one pass over the script (cheapest cases first in the emulator slice)"""
    d = c.desc
    per_row = d["conv1_kernel"] * 40 * d["conv1_filters"] + sum((k * ci if kind == "mix" else ci * co) for kind, k, ci, co, _ in layers_of(d))
    per_row += d["t_final"] * d["blocks"][-1][2]
    rows = 0
    for st in c.script:
        n = {"tracks": lambda: sum(st[1]) // d["stride"], "host": lambda: st[1] // d["stride"], "ones": lambda: st[1],
             "outputs": lambda: 2500 if st[1] == "grid" else st[1]}.get(st[0], lambda: 0)()
        rows += n + (reach1_of(d) * (1 + n // TILE) if n else 0)
    return per_row * (rows + 4 * c.cap)


def emulator_slice():
    """every item once, cheapest cases first (greedy): the part of the plan the CPU suite runs through the emulated kernels"""
    need, out = set(required()), []
    for c in sorted(_cases(), key=cost):
        got = items_of(c) & need
        if got:
            out.append(c)
            need -= got
    assert not need, need
    return out


# ------------------------------------------------------------------------------------------------------ running
class _Session:
    """one stream (float or int8) of a case driven through the script, every call held to the oracle"""

    def __init__(self, lib, b, kind, seed, n_cu, stores, worst):
        from microwakeword_amd import native, streaming
        self.b, self.kind, self.seed, self.n_cu, self.stores, self.worst = b, kind, seed, n_cu, stores, worst
        self.model = sc.context_model(lib)
        if kind == "float":
            self.st = native.Stream(self.model.engine, b.desc)
            self.st.set_weights(b.flat)
        else:
            self.qsm = streaming.QuantizedStreamingModel(b.qm, b.s, "stream", context=self.model)
            self.st = self.qsm.native
        self._reset_oracle()

    def _reset_oracle(self):
        self.fed, self.only_ones = [], True
        self.step = so.StepStream(self.b.net) if self.kind == "float" else qo.StepStreamQ8(self.b.qm)

    def _state(self):
        return self.st.get_state() if self.kind == "float" else self.st.get_state_q8()

    def _check(self, n_new, what, step_ref=None):
        """the last call's n_new outputs and the state against the oracle over everything fed since the reset"""
        b = self.b
        if self.kind == "float":
            p, z = self.st.read(want_logits=True)
            assert p.size == n_new, (what, p.size, n_new)
            if step_ref is not None:
                ref_z, ref_st = step_ref
            else:
                ref_z, ref_st = so.whole_sequence(b.net, np.concatenate(self.fed, 0), rings=True)
                ref_z = ref_z[ref_z.size - n_new:]
            sc._compare(p, z, ref_z, what)
            if n_new:
                self.worst["logit"] = max(self.worst["logit"], float(np.abs(z - ref_z).max()))
            self.worst["state"] = max(self.worst["state"], sc.compare_state(self._state(), ref_st, b.net, what))
        else:
            u8 = self.st.read_q8()
            assert u8.size == n_new, (what, u8.size, n_new)
            if step_ref is not None:
                ref_lq, ref_st = step_ref
                ref_u8 = b.qm.lut[np.asarray(ref_lq, np.int64) + 128]
            else:
                ref_u8, ref_lq, ref_st = qo.whole_sequence(b.qm, np.concatenate(self.fed, 0))
                ref_u8, ref_lq = ref_u8[ref_u8.size - n_new:], ref_lq[ref_lq.size - n_new:]
            lq = self.st.read(want_logits=True)[1]
            assert np.array_equal(u8, ref_u8), "%s: %d of %d uint8 outputs differ (%d int8 logits)" % (
                what, int(np.sum(u8 != ref_u8)), u8.size, int(np.sum(lq != np.asarray(ref_lq, np.float32))))
            qc.check_logits(self.qsm, ref_lq, what)
            got_st = self._state()
            assert np.array_equal(got_st, ref_st), "%s: rings differ at %s" % (what, np.nonzero(got_st != ref_st)[0][:8])
            qc._check_probs(self.qsm, u8)

    def run(self, i):
        b, s = self.b, self.b.s
        st = b.case.script[i]
        what = "%s %s step %d %s" % (b.case.id, self.kind, i, st[0])
        rng = _rng(b.case.id, self.seed, i)
        if st[0] == "reset":
            self.st.reset()
            self._reset_oracle()
        elif st[0] == "zero":
            before = self._state()
            n = self.st.run_host(gen_frames(rng, s - 1))
            assert n == 0 and self.st.n_out == 0, what
            assert np.array_equal(before.view(np.uint8), self._state().view(np.uint8)), what + ": a call without outputs changed the state"
        elif st[0] == "tracks":
            tr = sc.Tracks(self.model, st[1], st[2], seed=int(rng.integers(1 << 30)), store_ids=self.stores)
            off = self.st.run(tr.win)
            for t, L in enumerate(st[1]):
                assert off[t + 1] - off[t] == L // s, what
            self.fed += [f[:(len(f) // s) * s] for f in tr.frames]
            self.only_ones = False
            self._check(int(off[-1]), what)
        elif st[0] in ("host", "outputs"):
            if st[0] == "host":
                L = st[1]
            else:
                L = ((2 * self.n_cu + 2) * TILE + 5 if st[1] == "grid" else st[1]) * s + (s - 1)   # trailing frames are dropped
            x = gen_frames(rng, L, "u16" if i % 2 else "f32")
            n = self.st.run_host(x)
            assert n == L // s, what
            self.fed.append(x[:(L // s) * s])
            self.only_ones = False
            self._check(n, what)
        elif st[0] == "ones":
            for j in range(st[1]):
                x = gen_frames(rng, s)
                assert self.st.run_host(x) == 1, what
                self.fed.append(x)
                ref = None
                if self.only_ones:   # the literal ring form, one step per chunk
                    lz = self.step.step(x)
                    ref = (np.array([lz]), self.step.state())
                self._check(1, "%s call %d" % (what, j), ref)
        else:
            raise ValueError(st)

    def close(self):
        self.st.close()


def _splits(rng, n_out, s):
    """three random splits of n_out outputs into calls, each with one-output and zero-output calls"""
    out = []
    for _ in range(3):
        cuts = sorted(int(v) for v in rng.choice(np.arange(1, n_out - 1), 6, replace=False))
        cuts = sorted(set(cuts) | {cuts[2] + 1})                 # a one-output call
        bounds = [0] + cuts + [cuts[-1]] + [n_out]               # a zero-output call (an empty piece)
        bounds.insert(2, bounds[1])
        out.append([(a * s, b * s) for a, b in zip(bounds, bounds[1:])])
    return out


def _chunking(lib, b, kind, worst):
    """any split of the sequence into calls gives bit for bit the probabilities and the final state of one call; a second
    run of the one call does too; for the float kernel the REC form on the same sequence as well, with its ranges held
    as q8_checks.check_calibration holds them"""
    from microwakeword_amd import native, streaming
    model = sc.context_model(lib)

    def fresh():
        if kind == "float":
            st = native.Stream(model.engine, b.desc)
            st.set_weights(b.flat)
            return st
        return streaming.QuantizedStreamingModel(b.qm, b.s, "stream", context=model).native

    def state(st):
        return (st.get_state() if kind == "float" else st.get_state_q8()).view(np.uint8)

    n_out = len(b.seq) // b.s
    st = fresh()
    assert st.run_host(b.seq) == n_out
    p0, z0 = st.read(want_logits=True)
    s0 = state(st)
    st.close()
    st = fresh()   # two-run bit equality
    st.run_host(b.seq)
    assert np.array_equal(st.read().view(np.uint32), p0.view(np.uint32)) and np.array_equal(state(st), s0), b.case.id + ": reruns differ"
    st.close()
    for si, pieces in enumerate(_splits(_rng(b.case.id, 77), n_out, b.s)):
        st = fresh()
        ps = []
        for lo, hi in pieces:
            n = st.run_host(b.seq[lo:hi])
            assert n == (hi - lo) // b.s
            ps.append(st.read())
        assert np.array_equal(np.concatenate(ps).view(np.uint32), p0.view(np.uint32)), "%s %s split %d %s: probabilities differ" % (
            b.case.id, kind, si, pieces)
        assert np.array_equal(state(st), s0), "%s %s split %d %s: final state differs" % (b.case.id, kind, si, pieces)
        st.close()
    if kind == "float":
        st = fresh()
        ranges = st.calibrate_host(b.seq)
        assert ranges.shape == (len(layers_of(b.desc)) + 3, 2)
        assert np.array_equal(st.read().view(np.uint32), p0.view(np.uint32)), b.case.id + ": REC changes the probabilities"
        assert np.array_equal(state(st), s0), b.case.id + ": REC changes the state"
        st.close()
        assert ranges[-1, 0] == z0.min() and ranges[-1, 1] == z0.max()
        assert ranges[0, 0] == b.seq.min() and ranges[0, 1] == b.seq.max()
        ref = qc.float64_ranges(b.om, b.flags, b.seq)
        for t, (got, want) in enumerate(zip(ranges.astype(np.float64), ref)):
            mag = max(abs(want[0]), abs(want[1]), 1e-30)
            assert np.all(np.abs(got - want) <= qc.RANGE_RTOL * mag), (b.case.id, "range of tensor %d" % t, got, want)


def _non_stream(lib, b, worst):
    from microwakeword_amd import native
    model = sc.context_model(lib)
    lens, pads = b.case.ns
    # float: against the non-streaming oracle model on every window
    st = native.Stream(model.engine, dict(b.desc, mode="non_stream"))
    st.set_weights(b.flat)
    tr = sc.Tracks(model, lens, pads, seed=SEED)
    off = st.run(tr.win)
    p, z = st.read(want_logits=True)
    for t, f in enumerate(tr.frames):
        ref = so.non_stream_windows(b.om, f.astype(np.float64), b.T, b.s)
        sc._compare(p[off[t]:off[t + 1]], z[off[t]:off[t + 1]], ref, "%s non_stream track %d" % (b.case.id, t))
        if ref.size:
            worst["logit"] = max(worst["logit"], float(np.abs(z[off[t]:off[t + 1]] - ref).max()))
    st.close()
    # int8: against the integer oracle, and stream mode against non_stream mode past the warm-up
    qc.check_q8_non_stream(lib, b.flags, b.T, lens, pads, seed=SEED, qm=b.qm, model=model)
    qc.check_stream_equals_non_stream_past_warmup(model, b.qm, b.flags, b.T, [b.T + 40, 3 * b.T + 7])


def run_case(lib, c, n_cu=256, kinds=("float", "q8")):
    """one case through the float kernel, its REC form and the int8 kernel; returns the figures of the results file"""
    b = built(c.id)
    t0 = time.time()
    worst = {"logit": 0.0, "state": 0.0}
    if "q8" in kinds and c.spread:
        qc.check_spread(b.qm, b.seq, c.id)   # a condition on the inputs: before any kernel runs
    for kind in kinds:
        sessions = [_Session(lib, b, kind, 0, n_cu, (0, 1), worst)] + ([_Session(lib, b, kind, 1, n_cu, (2, 3), worst)] if c.two else [])
        for i in range(len(c.script)):
            for ses in sessions:   # two streams of one context, alternately: independent rings
                ses.run(i)
        for ses in sessions:
            ses.close()
        _chunking(lib, b, kind, worst)
    if kinds == ("float", "q8"):
        _non_stream(lib, b, worst)
    return dict(id=c.id, seconds=time.time() - t0, logit_err=worst["logit"], state_err=worst["state"],
                logit_ratio=worst["logit"] / ec.FWD_TOL, state_ratio=worst["state"] / ec.FWD_TOL,
                branches=sorted(oracle_report(c.id)[1]))
