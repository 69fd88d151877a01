"""A covering sweep of the conv/BN graph streaming kernels - ``stream_graph_kernel<false>`` with its calibration form
``<REC = true>`` (csrc/tu_stream_graph.hip) and ``stream_graph_q8_kernel`` (csrc/tu_stream_graph_q8.hip), both driven by
``Graph::plan`` - shared by the GPU sweep (tests/test_stream_graph_sweep_gpu.py) and its CPU-side checks
(tests/test_stream_graph_sweep_emulated.py).  The shape of tests/stream_sweep.py, for the other run-time-shape family.

``Graph::plan`` accepts any DAG of up to 48 convolutions, each with one to three sources that are channel slices of an
earlier op or of the spectrogram, kernel / dilation / filters in 1..1024 and any bn_groups that divides the filters; it
places the tensors with a first-fit arena by liveness and derives every barrier flag, once in floats and once in bytes.
The realistic tests run Inception topologies only.  So:

- ``cases()`` is a deterministic, seeded (SEED) list of small hand-written cases.  A case is a description built directly,
  random Keras-order weights for it (``quant_graph_oracle.random_weights``, BatchNorm statistics from a float64 dry run), a
  stream-mode call script in the vocabulary of ``stream_sweep.Case`` and a non-stream twin.  What a case covers is COMPUTED
  (``items_of``) from its description, its script, an oracle dry run and ``Plan`` - a Python restatement of the geometry of
  ``Graph::plan`` (lengths, reach, ring layout, the arena and the barrier rule in floats and in bytes, the int8 tile) that is
  held to the library wherever the library exposes a number (``check_geometry``).  The barrier flags are not exported: the
  restated ones only decide which case covers which item.
- ``required()`` lists the items; ``uncovered()`` must equal ``UNREACHABLE`` (each entry with its reason).
- ``run_case(lib, case)`` drives one case through the float kernel, its REC form and the int8 kernel and holds every call
  to tests/stream_graph_oracle.py (float64) and tests/quant_graph_oracle.py (integers): outputs, logits AND rings.
- three conditions on a case's INPUTS come from the oracles alone: ``float32_condition`` (the float32 restatement within
  CONDITION of each bound of the float64 one), ``quant_graph_checks.check_spread`` and ``sensitivity`` (dropping any one
  source of a multi-source op or any one tap of a k > 1 op moves a float64 logit by more than twice FWD_TOL and changes an
  int8 logit: a slice or ring bug cannot hide under the tolerance).
"""
import functools
import time
import types

import numpy as np

import engine_checks as ec
import q8_checks as qc
import quant_graph_checks as qgc
import quant_graph_oracle as qgo
import quant_oracle as qo
import stream_graph_oracle as sgo
import stream_sweep as ss
import streaming_checks as sc

SEED = 2027
TILE = ss.TILE
KMAX_LDS = ss.KMAX_LDS
CHAIN_MAX_RING = ss.CHAIN_MAX_RING
CONDITION = 0.25          # share of a bound the float32 restatement may use up
MAX_OPS, MAX_SOURCES = 48, 3   # MWW_MAX_GRAPH_OPS, MWW_MAX_OP_SOURCES of include/mww.h
BINS = 40


def r4(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------------------------------------- descriptions
def op(src, k=1, d=1, f=4, g=1, sl=None):
    src = list(src)
    return dict(src=src, drop=[0] * len(src), slice=[tuple(s) for s in (sl or [(0, 0)] * len(src))], kernel=k, dilation=d, filters=f,
                bn_groups=g)


def desc_of(ops, tf):
    """the description of ``ops`` whose final map has ``tf`` frames: ``drop`` aligns the sources of every op to the shortest
    (what StridedDrop states in the non-streaming model) and ``frames`` is the window that leaves tf final frames"""
    ops = [dict(o) for o in ops]
    short = [0]   # frames a tensor is shorter than the window; tensor 0 is the spectrogram
    for o in ops:
        m = max(short[s + 1] for s in o["src"])
        o["drop"] = [m - short[s + 1] for s in o["src"]]
        short.append(m + (o["kernel"] - 1) * o["dilation"])
    frames = tf + short[-1]
    assert frames - max(short) >= 1, "an op nobody reads is left without a frame: raise tf"
    return dict(conv_ops=ops, op_names=["op%d" % i for i in range(len(ops))], frames=frames, stride=1, mode="stream")


# ------------------------------------------------------------------------------- Graph::plan's geometry, restated
class Plan:
    """what ``Graph::plan`` (csrc/tu_stream_graph.hip) derives from a description: the refusal it would answer, else lengths,
    rings, reach, sizes and the two placements"""

    def __init__(self, desc, tile=TILE):
        self.refusal = self._geometry(desc)
        if self.refusal is None:
            self.f32 = self._place(tile, False)
            self.q8 = self._place(tile, True)
            self.tile_bytes = self.q8.top

    def _geometry(self, desc):
        ops, T = desc["conv_ops"], int(desc["frames"])
        n = self.n = len(ops)
        if n <= 0 or n > MAX_OPS:
            return "n_ops must be 1..%d" % MAX_OPS
        if T <= 0:
            return "frames must be positive"
        self.len, self.ch, self.R, self.cin, self.src, self.k, self.cout = [], [], [], [], [], [], []
        self.last_use = [-1] * n
        kw = qw = 0
        for i, o in enumerate(ops):
            k, d, f, g = int(o["kernel"]), int(o.get("dilation", 1)), int(o["filters"]), int(o.get("bn_groups", 1))
            for name, v in (("kernel", k), ("dilation", d), ("filters", f)):
                if v <= 0 or v > 1024:
                    return "op %d: %s must be 1..1024" % (i, name)
            if g <= 0 or f % g:
                return "op %d: bn_groups must divide the filters" % i
            if not 0 < len(o["src"]) <= MAX_SOURCES:
                return "op %d: n_src must be 1..3" % i
            tin, cin, srcs = -1, 0, []
            for j, (s, dr, (c0, cn)) in enumerate(zip(o["src"], o.get("drop", [0] * len(o["src"])), o.get("slice", [(0, 0)] * len(o["src"])))):
                if s < -1 or s >= i:
                    return "op %d: src must name an earlier op or -1" % i
                sl, sch = (T, BINS) if s < 0 else (self.len[s], self.ch[s])
                if dr < 0 or dr >= sl:
                    return "op %d: src_drop must leave at least one frame" % i
                if j and sl - dr != tin:
                    return "op %d: src_drop does not align the sources to one length" % i
                tin = sl - dr
                cn = cn if cn else sch - c0
                if c0 < 0 or cn <= 0 or c0 + cn > sch:
                    return "op %d: src_c0 / src_cn is not a slice of the source" % i
                srcs.append((s, c0, cn, sch))
                cin += cn
                if s >= 0:
                    self.last_use[s] = i
            R = (k - 1) * d
            if tin - R <= 0:
                return "op %d: kernel does not fit frames = %d (the window is too short for this graph)" % (i, T)
            self.len.append(tin - R)
            self.ch.append(f)
            self.R.append(R)
            self.cin.append(cin)
            self.src.append(srcs)
            self.k.append(k)
            self.cout.append(f)
            kw += k * cin * f + 4 * (g if g > 1 else f)
            qw += f * k * sum(r4(cn) for _, _, cn, _ in srcs)
        self.tf, self.c_last = self.len[-1], self.ch[-1]
        if self.tf * self.c_last > 1 << 24:
            return "frames leaves a final map too large for the head"
        self.n_weights = kw + self.tf * self.c_last + 1
        self.n_state = sum(r * c for r, c in zip(self.R, self.cin)) + (self.tf - 1) * self.c_last
        self.q8_sizes = (qw + self.tf * r4(self.c_last), 3 * sum(self.cout) + 3 + n + 2)
        self.num_tensors = n + 2
        # reach: frames between a tensor's rows and the first head input of a tile; candidates[t]: what each consumer asks of t
        self.reach = [0] * n
        self.reach[-1] = self.tf - 1
        self.in_reach = 0
        self.asked = {t: [] for t in range(-1, n)}
        for i in range(n - 1, -1, -1):
            for s, _, _, _ in self.src[i]:
                want = self.reach[i] + self.R[i]
                self.asked[s].append((i, want))
                if s < 0:
                    self.in_reach = max(self.in_reach, want)
                else:
                    self.reach[s] = max(self.reach[s], want)
        if self.in_reach > T - 1:
            return "frames is shorter than the graph's receptive field"
        self.in_last = max(i for i in range(n) if any(s < 0 for s, _, _, _ in self.src[i]))
        return None

    def _place(self, tile, in_bytes):
        """one pass of the planner's first-fit arena and barrier rule (floats, or bytes with rows of pitch r4(C)): offsets,
        sizes, barrier flags with what asked for each (output read / output written / a source written since the last
        barrier), which outputs landed in a freed buffer, the arena's top"""
        n, p = self.n, types.SimpleNamespace()
        free, top = [], [0]

        def take(sz):
            for e in free:
                if e[1] >= sz:
                    off = e[0]
                    e[0] += sz
                    e[1] -= sz
                    if not e[1]:
                        free.remove(e)
                    return off, True
            top[0] += sz
            return top[0] - sz, False

        def give(off, sz):
            free.append([off, sz])
            free.sort()
            i = 0
            while i + 1 < len(free):
                if free[i][0] + free[i][1] == free[i + 1][0]:
                    free[i][1] += free[i + 1][1]
                    del free[i + 1]
                else:
                    i += 1

        def hits(v, off, sz):
            return any(off < a + b and a < off + sz for a, b in v)

        in_size = (tile + self.in_reach) * BINS
        p.in_buf = take(in_size)[0]
        rd, wr = [], [(p.in_buf, in_size)]
        p.buf, p.size, p.sync, p.reused, p.why = [], [], [], [], []
        for i in range(n):
            size = (tile + self.reach[i]) * (r4(self.cout[i]) if in_bytes else self.cout[i])
            off, reused = take(size)
            p.buf.append(off)
            p.size.append(size)
            p.reused.append(reused)
            srcs = [(p.in_buf, in_size) if s < 0 else (p.buf[s], p.size[s]) for s, _, _, _ in self.src[i]]
            why = (hits(rd, off, size), hits(wr, off, size), any(hits(wr, a, b) for a, b in srcs))
            p.why.append(why)
            p.sync.append(int(any(why)))
            if any(why):
                rd, wr = [], []
            wr.append((off, size))
            rd += srcs
            if self.in_last == i:
                give(p.in_buf, in_size)
            for t in range(i):
                if self.last_use[t] == i:
                    give(p.buf[t], p.size[t])
            if self.last_use[i] < 0 and i != n - 1:
                give(off, size)
        p.top = top[0]
        return p


@functools.lru_cache(maxsize=None)
def plan_of(cid):
    return Plan(case(cid).desc)


def _tile_bytes(desc):
    pl = Plan(desc)
    return pl.tile_bytes if pl.refusal is None else None


def tile_placement(pl):
    if pl.tile_bytes > KMAX_LDS:
        return "scratch"
    return "lds<64K" if pl.tile_bytes <= 64 * 1024 else "lds-64K-160K"


def _widened(desc, by):
    """the description with its largest tensor's op ``by`` filters wider (a pitch step of the int8 tile)"""
    pl = Plan(desc)
    i = int(np.argmax(pl.q8.size))
    ops = [dict(o) for o in desc["conv_ops"]]
    ops[i]["filters"] += by
    return dict(desc, conv_ops=ops)


def check_geometry(lib, c):
    """the restatement against every number the library exposes: n_weights, n_state, num_tensors, q8_sizes, in both modes"""
    from microwakeword_amd import native
    model = sc.context_model(lib)
    pl = plan_of(c.id)
    assert pl.refusal is None, pl.refusal
    for mode in ("stream", "non_stream"):
        for int8 in (False, True):
            st = native.GraphStream(model.engine, dict(c.desc, mode=mode), int8=int8)
            assert st.n_weights == pl.n_weights == built(c.id).flat.size, (c.id, st.n_weights, pl.n_weights)
            assert st.n_state == pl.n_state == built(c.id).net.n_state(), (c.id, st.n_state, pl.n_state)
            if int8:
                assert st.num_tensors() == pl.num_tensors and st.q8_sizes() == pl.q8_sizes, (c.id, st.q8_sizes(), pl.q8_sizes)
            st.close()
    w, iv, _, _ = built(c.id).qm.packed()
    assert (w.size, iv.size) == pl.q8_sizes, (c.id, w.size, iv.size, pl.q8_sizes)


# ------------------------------------------------------------------------------------------------------- cases
class Case:
    """``script`` / ``two``: as ``stream_sweep.Case`` (the stride is 1: a "zero" step is a call of no frames).  ``ns``:
    (lengths, pads) of the non-stream twin, the same description in non_stream mode.  ``w_edit`` / ``r_edit`` / ``i_edit``:
    the hand edits of the dedicated requantization cases (float weights, calibrated ranges, int32 values).  ``bn_shift`` /
    ``dense_scale`` scale the random weights so that the float32 restatement stays within CONDITION of the bounds;
    ``tap_floor`` keeps every kernel value at least that many standard deviations from zero (the sensitivity condition of a
    kernel with a thousand taps: the smallest of a thousand normal values is too close to zero to show)."""

    def __init__(self, cid, desc, script=None, ns=None, two=False, w_edit=None, r_edit=None, i_edit=None, spread=True, cap=400,
                 bn_shift=0.0, dense_scale=1.0, tap_floor=0.0):
        self.id, self.desc, self.two = cid, desc, two
        T = desc["frames"]
        pl = Plan(desc)
        assert pl.refusal is None, (cid, pl.refusal)
        chain = max(pl.R + [pl.tf - 1]) + 2
        self.script = script if script is not None else [
            ("tracks", [0, 7, T + 5, 0, 3, 2 * T + 2, 0], [0, 2, 0, 0, 0, 4, 0]),
            ("zero",),
            ("host", T + 9),
            ("reset",),
            ("ones", chain if chain - 2 <= CHAIN_MAX_RING else 3),
            ("tracks", [301, 2], [0, 0]),
        ]
        self.ns = ns if ns is not None else ([T, T - 1, 0, T + 4], [T // 2, 0, 0, 0])
        self.w_edit, self.r_edit, self.i_edit, self.spread = w_edit, r_edit, i_edit, spread
        self.bn_shift, self.dense_scale, self.tap_floor, self.cap = bn_shift, dense_scale, tap_floor, cap
        assert spread == ("nospread" not in cid)   # a case that cannot reach the spread condition says so in its id

    def __repr__(self):
        return self.id


def _zero_and_tiny_channels(w):
    """float-weight edit: an all-zero output channel of op 1 (weight scale 1) and one with tiny weights (an effective
    multiplier below 2^-16: right shifts >= 16)"""
    w[5] = w[5].copy()
    w[5][..., 1] = 0.0
    w[5][..., 2] *= 1e-5
    return w


def _unnormalised_multipliers(qm):
    """int32 edit: the same effective multipliers written with a LEFT shift (M >> k, shift + k: the device takes any
    M >= 0), and the two shift edges on one channel each"""
    o = qm.ops[1]
    for c in (0, 3, 4):
        k = 2 - int(o["shift"][c])
        assert 0 < k < 20
        o["multiplier"][c] >>= k
        o["shift"][c] += k
    o["shift"][5], o["shift"][6] = -31, 30
    d = qm.ops[-1]   # the Dense too: a left shift on the logit's own requantization
    k = 1 - int(d["shift"][0])
    assert 0 < k < 20
    d["multiplier"][0] >>= k
    d["shift"][0] += k


def cases():
    """the plan: small cases, each built around the axes its id names"""
    out = []
    # every kind of source in one graph: slices on and off the word grid with widths 1, 2, 3 mod 4, one that ends at the end of
    # a 10-channel row (its two padding bytes are never written), the spectrogram read through a slice by op 3 next to an op's
    # output, op 0 read by ops 1, 2 and 5 (op 2's path is the longest: the maximum is neither the first nor the last candidate
    # the planner meets), twice by op 5, op 4 read by nobody, and op 6's ring made of three sources 9 + 6 + 8 wide
    out.append(Case("sources_slices_diamond_unread", desc_of([
        op([-1], k=3, f=10, g=2),
        op([0], f=7, g=7, sl=[(4, 5)]),
        op([0], k=3, d=2, f=9, g=3, sl=[(3, 7)]),
        op([-1, 1], k=2, f=6, sl=[(6, 6), (0, 0)]),
        op([2], k=2, f=5, g=5),
        op([0, 0], f=8, sl=[(0, 3), (8, 2)]),
        op([2, 3, 5], k=3, f=11)], 3), two=True))
    # the arena and the barrier rule: op 2 reads the spectrogram late (in_buf is given back after op 2, not after op 0) into the
    # buffer op 0 left, which op 1 has read since the last barrier: a barrier that no written source asks for.  Ops 3 and 4
    # share an interval.  Widths 6 and 7 have one byte pitch: the byte plan reuses where the float plan cannot.
    out.append(Case("arena_late-input_out-read-only", desc_of([
        op([-1], k=2, f=6),
        op([0], k=2, f=7, g=7),
        op([-1], f=6, g=2, sl=[(1, 38)]),
        op([1], f=7),
        op([1, 2], k=3, f=5, sl=[(0, 0), (2, 3)]),
        op([3, 4], k=2, f=9, g=3),
        op([5], f=3)], 2)))
    # the two plans part: op 2 (7 wide: 7 floats, 8 bytes a row) fits the buffer op 0 (6 wide: 6 floats, 8 bytes) left only in the
    # byte plan, where op 1 has read that buffer since the last barrier: the byte plan reuses and sets a barrier, the float plan
    # does neither
    out.append(Case("arena_plans-differ", desc_of([
        op([-1], k=2, f=6, g=3),
        op([0], f=5),
        op([-1], f=7, sl=[(20, 20)]),
        op([1, 2], k=2, f=4, g=2)], 2)))
    # the limits, accepted just inside: kernel 1024 on a one-channel slice with one filter (a one-op graph, a ring longer than a
    # tile from a large kernel, cin = cout = c_last = 1); every call is shorter than the ring
    out.append(Case("k1024_one-op_cin1_cout1", desc_of([op([-1], k=1024, f=1, sl=[(5, 1)])], 2),
                    script=[("tracks", [0, 300, 0, 41], [0, 5, 0, 0]), ("zero",), ("host", 700), ("outputs", 257), ("reset",), ("ones", 3),
                            ("host", 1100)], ns=([1025, 1024, 0, 1030], [100, 0, 0, 0]), cap=1300, tap_floor=1.0))
    # dilation 1024 with k = 2 (a ring longer than a tile from a large dilation), t_final = 1: no head ring
    out.append(Case("d1024_k2_tf1", desc_of([op([-1], f=2, g=2, sl=[(0, 6)]), op([0], k=2, d=1024, f=3, g=3)], 1),
                    script=[("tracks", [0, 500, 3], [0, 0, 0]), ("zero",), ("host", 600), ("reset",), ("ones", 3), ("outputs", 513)],
                    ns=([1025, 1024, 0, 1029], [7, 0, 0, 0]), cap=1300))
    # 48 ops in a chain (MWW_MAX_GRAPH_OPS), every fourth with a ring; 48 ReLU layers of random weights are chaotic, so the
    # BatchNorm offsets keep most units on the linear side (as stream_sweep's layers128 case)
    chain = [op([i - 1], k=2 if i % 4 == 1 else 1, f=3 + i % 3, g=1 if i % 2 else 3 + i % 3) for i in range(48)]
    out.append(Case("chain48", desc_of(chain, 2), bn_shift=2.0, dense_scale=0.1, cap=300))
    # only k = 1 ops: the state is the head ring alone
    out.append(Case("k1-only", desc_of([op([-1], f=5), op([0, -1], f=6, g=2, sl=[(0, 0), (36, 4)]), op([1], f=2, g=2)], 4), cap=300))
    # a head over more frames than a tile has outputs: the head ring and the halo are longer than a tile
    out.append(Case("tf300", desc_of([op([-1], k=2, f=3, sl=[(8, 9)])], 300),
                    script=[("tracks", [0, 100, 320, 0], [0, 5, 0, 0]), ("zero",), ("outputs", 257), ("reset",), ("ones", 3), ("outputs", 330)],
                    cap=700))
    # 1024 filters, and a final map of 256 x 1024 values = 2^18.  The limit is 2^24; a call of n outputs costs
    # (n + 255) * 40 * 1024 + n * 2^18 multiply-adds whatever n is, the checks make some forty calls, and this case runs in the
    # emulator slice: 2^18 is what that affords (2^24 would be 64 times the head and 16 times the halo)
    out.append(Case("w1024_final-map-2^18", desc_of([op([-1], f=1024, g=2)], 256),
                    script=[("tracks", [0, 9, 0], [0, 2, 0]), ("zero",), ("host", 70), ("reset",), ("ones", 2)], ns=([256, 255, 0, 258], [5, 0, 0, 0]),
                    cap=80))
    # int8 tile placement: 10 360 B of input rows + 259 rows of the wide tensor; 300 wide: between 64 KB and 160 KB; 592 wide:
    # 163 688 B, the largest that fits 160 KB; 596 wide: 164 724 B, the smallest that does not.  The wide op is k = 1 and is read
    # through a five-channel slice, so the width costs only its own rows.
    for cid, w, g in (("lds-mid_w300", 300, 1), ("lds-largest_w592", 592, 2), ("scratch-smallest_w596", 596, 1)):
        out.append(Case(cid, desc_of([op([-1], f=w, g=g), op([0], k=3, f=6, sl=[(w - 9, 5)])], 2),
                        script=[("tracks", [0, 30, 0], [0, 3, 0]), ("zero",), ("host", 261), ("reset",), ("ones", 3)], cap=120))
    # exact tile boundaries and more tiles than 2 x CU workgroups (the grid-stride loop) on a one-filter graph; more than 256
    # windows behind a short track in the twin
    out.append(Case("grid-stride_tile-edges_f1", desc_of([op([-1], k=2, f=1, sl=[(3, 4)])], 2),
                    script=[("outputs", 255), ("outputs", 256), ("zero",), ("outputs", 257), ("outputs", 513), ("outputs", "grid"),
                            ("reset",), ("ones", 4), ("outputs", 256)], ns=([3, 2, 5, 0, 262 + 3], [0, 0, 1, 0, 0])))
    out.append(Case("ns-windows_f2", desc_of([op([-1], k=2, f=2, g=2, sl=[(0, 7)]), op([0, -1], k=2, f=2, sl=[(0, 0), (30, 3)])], 2),
                    ns=([4, 3, 0, 2, 300], [1, 0, 0, 0, 0])))
    # drops beyond what aligning the sources needs (a StridedDrop of one more leading frame on both sources of op 1, one on the
    # single source of op 2): the window grows by those frames, the stream form is the same graph
    d = desc_of([op([-1], k=2, f=4, g=2), op([0, -1], k=2, f=3, sl=[(1, 3), (10, 6)]), op([1], k=2, f=2)], 2)
    d["conv_ops"][1]["drop"] = [v + 1 for v in d["conv_ops"][1]["drop"]]
    d["conv_ops"][2]["drop"] = [1]
    out.append(Case("extra-drop", dict(d, frames=d["frames"] + 2), cap=200))
    # the dedicated requantization cases: ranges and int32 values edited by hand (the oracle follows whatever they say)
    base = desc_of([op([-1], k=3, f=8), op([0], k=3, d=2, f=8, g=2), op([1], f=6, sl=[(2, 5)])], 3)
    out.append(Case("rq-ranges", base, w_edit=_zero_and_tiny_channels,
                    r_edit={0: ("set", 5.0, 30.0),      # the input saturates at both ends
                            1: ("neg-min", 0.3, 0.4),   # zero point above -128 and a short range: the ReLU clamp and 127
                            2: ("sym",),                # zero point 0
                            4: ("scale", 0.3),          # the logit (no ReLU) clamps at -128 and at 127
                            }))
    out.append(Case("rq-shifts_nospread", base, i_edit=_unnormalised_multipliers, spread=False,
                    r_edit={2: ("neg",),                # an output whose range ends at 0: zero point 127
                            3: ("set", 0.0, 0.0),       # a tensor of range (0, 0): scale 1, zero point 0
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


gen_frames = ss.gen_frames


def _conditioned_weights(desc, frames, seed, bn_shift, dense_scale, tap_floor=0.0):
    """``quant_graph_oracle.random_weights`` with the BatchNorm moving statistics := the statistics of each convolution's
    output on a float64 dry run over ``frames`` from zero rings (what training leaves there), and a Dense of unit scale"""
    w = [np.asarray(a, np.float64) for a in qgo.random_weights(desc, seed)]
    x = np.asarray(frames, np.float64)
    N, tensors = x.shape[0], [x]
    for i, (o, srcs) in enumerate(zip(desc["conv_ops"], qgo.qg.op_sources(desc))):
        k, d, co, g = int(o["kernel"]), int(o.get("dilation", 1)), int(o["filters"]), int(o.get("bn_groups", 1))
        a = np.concatenate([tensors[t][:, c0:c0 + cn] for t, c0, cn in srcs], 1)
        a = np.concatenate([np.zeros((d * (k - 1), a.shape[1])), a], 0)
        if tap_floor:
            w[5 * i] = np.sign(w[5 * i]) * (np.abs(w[5 * i]) + tap_floor * w[5 * i].std())
        kern = w[5 * i].reshape(k, a.shape[1], co)
        y = np.zeros((N, co))
        for j in range(k):
            y = y + a[j * d:j * d + N] @ kern[j]
        slots = g if g > 1 else co
        cols = [y[:, s::slots] for s in range(slots)]   # channel c in slot c mod g
        mean, var = np.array([c.mean() for c in cols]), np.array([c.var() for c in cols])
        var = np.where(var > 1e-12, var, 1.0)
        w[5 * i + 3], w[5 * i + 4] = mean - bn_shift * np.sqrt(var), var
        slot = np.arange(co) % slots
        tensors.append(np.maximum((y - w[5 * i + 3][slot]) / np.sqrt(var[slot] + sgo.BN_EPS) * w[5 * i + 1][slot] + w[5 * i + 2][slot], 0))
    rng = np.random.default_rng(seed + 1000)
    nd = qgo.final_frames(desc) * int(desc["conv_ops"][-1]["filters"])
    w += [rng.normal(0, dense_scale / np.sqrt(nd), (nd, 1)), rng.normal(0, 0.1, 1)]
    return [a.astype(np.float32) for a in w]


class Built:
    """everything derived from a case without a kernel"""


@functools.lru_cache(maxsize=None)
def built(cid):
    from microwakeword_amd import quantize_graph
    c = case(cid)
    b = Built()
    b.case, b.desc, b.T = c, c.desc, c.desc["frames"]
    b.seq = gen_frames(_rng(cid, 0), c.cap, "u16")
    b.seq[0, 0], b.seq[0, 1] = 0.0, 26.0
    if c.r_edit and 0 in c.r_edit:   # a case that narrows the input range also feeds rows below zero (saturation at -128)
        b.seq[5:50] -= np.float32(8.0)
    b.weights = _conditioned_weights(c.desc, b.seq, SEED, c.bn_shift, c.dense_scale, c.tap_floor)
    if c.w_edit:
        b.weights = c.w_edit(b.weights)
    b.net = sgo.Net(c.desc, b.weights)
    b.flat = np.concatenate([w.reshape(-1) for w in b.weights])
    ranges = qgc.desc_ranges(c.desc, b.weights, b.seq)
    for t, e in (c.r_edit or {}).items():
        lo, hi = ranges[t]
        ranges[t] = {"set": lambda: (e[1], e[2]), "scale": lambda: (lo * e[1], hi * e[1]), "sym": lambda: (-max(-lo, hi), max(-lo, hi)),
                     "neg": lambda: (lo - 1.0, 0.0), "neg-min": lambda: (-e[1] * hi, e[2] * hi)}[e[0]]()
    b.qm = quantize_graph.quantize_weights(c.desc, b.weights, ranges.astype(np.float32))
    if c.i_edit:
        c.i_edit(b.qm)
    return b


def float32_condition(cid):
    """the float32 restatement against the float64 one over the case's sequence, as fractions of the bounds:
    (logits / FWD_TOL, probabilities / PROB_TOL, activation rings / FWD_TOL)"""
    b = built(cid)
    z64, st64 = sgo.whole_sequence(b.net, b.seq, rings=True)
    z32, st32 = sgo.whole_sequence(sgo.Net(b.desc, b.weights, dtype=np.float32), b.seq, rings=True)
    assert np.all(np.isfinite(z64)) and np.all(np.isfinite(st64))
    return (float(np.abs(z32 - z64).max()) / ec.FWD_TOL, float(np.abs(sgo.sigmoid(z32) - sgo.sigmoid(z64)).max()) / sc.PROB_TOL,
            (float(np.abs(st32 - st64).max()) if st64.size else 0.0) / ec.FWD_TOL)


def _float_from(net, i, y, tensors):
    """float64 logits with op i's output replaced by relu(y): the ops behind it re-run"""
    tensors = tensors[:i + 1] + [np.maximum(y, 0)]
    for o in range(i + 1, net.n):
        a = net.gather(o, tensors)
        tensors.append(net.conv(o, np.concatenate([np.zeros((net.ops[o]["R"], a.shape[1])), a], 0)))
    return net.head(np.concatenate([np.zeros((net.tf - 1, net.c_last)), tensors[-1]], 0))


def _q8_from(q, i, acc, tensors):
    """int8 logits with op i's accumulator replaced by acc"""
    tensors = tensors[:i + 1] + [qo.requant(acc, q.ops[i], q.zp[1 + i], True)]
    for o in range(i + 1, q.n):
        a = q.gather(o, tensors)
        tensors.append(q.conv(o, np.concatenate([np.tile(q.zp_row(o), (q.R[o], 1)), a], 0)))
    return q.head(np.concatenate([np.full((q.tf - 1, q.c_last), q.zp[q.n], np.int64), tensors[-1]], 0))


@functools.lru_cache(maxsize=None)
def sensitivity(cid):
    """for every (op, source) of a multi-source op and every (op, tap) of a k > 1 op: the largest float64 logit change over
    the case's sequence when that source's / tap's contribution is dropped, and the number of int8 logits that change.
    -> [(what, float change, int8 logits changed)].  Computed from the two oracles: the contribution is subtracted from the op's
    pre-activation sum (float64) / accumulator (integers) and everything behind the op is run again."""
    b = built(cid)
    net, N = b.net, len(b.seq)
    tensors = []
    z = sgo.whole_sequence(net, b.seq, tensors_out=tensors)
    q = qgo.Q(b.qm)
    qt = [qo.quantize_input(b.seq, q.scale0, q.zp[0])]
    for i in range(q.n):
        a = q.gather(i, qt)
        qt.append(q.conv(i, np.concatenate([np.tile(q.zp_row(i), (q.R[i], 1)), a], 0)))
    lq = q.head(np.concatenate([np.full((q.tf - 1, q.c_last), q.zp[q.n], np.int64), qt[-1]], 0))
    out = []
    live = {net.n - 1}   # ops the logit depends on (the output of an op nobody reads is held by the REC form alone)
    for i in range(net.n - 1, -1, -1):
        if i in live:
            live |= {t - 1 for t, _, _, _ in net.ops[i]["parts"] if t > 0}
    for i, o in enumerate(net.ops):
        if i not in live:
            continue
        a = net.gather(i, tensors)
        a = np.concatenate([np.zeros((o["R"], o["cin"])), a], 0)
        qa = np.concatenate([np.tile(q.zp_row(i), (q.R[i], 1)), q.gather(i, qt)], 0) - q.zp_row(i)[None, :]
        y = np.zeros((N, o["co"])) + o["b"]
        acc = np.zeros((N, o["co"]), np.int64) + q.ops[i]["bias"]
        parts_f, parts_q = [], []
        for j in range(o["k"]):
            rows = slice(j * o["d"], j * o["d"] + N)
            parts_f.append(a[rows] @ o["w"][j])
            parts_q.append(qo.imatmul(qa[rows], q.ops[i]["weights"][j]))
            y, acc = y + parts_f[-1], acc + parts_q[-1]
        drops = []
        if o["k"] > 1:
            drops += [("op %d tap %d" % (i, j), parts_f[j], parts_q[j]) for j in range(o["k"])]
        if len(o["parts"]) > 1:
            at = 0
            for s, (_, _, cn, _) in enumerate(o["parts"]):
                cols = slice(at, at + cn)
                df = sum(a[j * o["d"]:j * o["d"] + N, cols] @ o["w"][j][cols] for j in range(o["k"]))
                dq = sum(qo.imatmul(qa[j * o["d"]:j * o["d"] + N, cols], q.ops[i]["weights"][j][cols]) for j in range(o["k"]))
                drops.append(("op %d source %d" % (i, s), df, dq))
                at += cn
        for what, df, dq in drops:
            zf = _float_from(net, i, y - df, tensors)
            zq = _q8_from(q, i, acc - dq, qt)
            out.append((what, float(np.abs(zf - z).max()), int(np.sum(zq != lq))))
    return out


@functools.lru_cache(maxsize=None)
def oracle_report(cid):
    """what the int8 oracle does on the case's sequence: (spread triple, branches taken) - both from the oracle alone"""
    b = built(cid)
    with qo.record_branches() as seen:
        sp = qgc.spread(b.qm, b.seq)
        seen = set(seen)
    for o in b.qm.ops:
        w = np.abs(o["weights"].astype(np.int64).reshape(-1, o["weight_scales"].size)) if o["kind"] != "dense" else np.abs(o["weights"]).reshape(-1, 1)
        if np.any((w.max(axis=0) == 0) & (o["weight_scales"] == 1)):
            seen.add("zero-weight-channel")
    if np.any((b.qm.ranges[:, 0] == 0) & (b.qm.ranges[:, 1] == 0)):
        seen.add("range-0-0")
    return sp, frozenset(seen)


# ------------------------------------------------------------------------------------------------------- items
BRANCH_ITEMS = ss.BRANCH_ITEMS

# items of required() no description the library accepts can reach, each with the reason read from the code
UNREACHABLE = {
    "plan:in_reach>frames-1": "Graph::plan's last refusal (\"frames is shorter than the graph's receptive field\") asks for in_reach > frames - 1. "
                              "in_reach is the largest sum of R along a path from the spectrogram plus the reach of the path's last op "
                              "(t_final - 1 for the final op, 0 for an op nobody reads); every op on a path was accepted with "
                              "len = frames - (sum of R so far, raised by src_drop) >= 1, and t_final = len of the final op, so every such "
                              "sum is at most frames - 1: the description is refused at that op (\"kernel does not fit frames\") before "
                              "the reach is computed - the code's own comment says \"cannot happen with aligned sources\"",
}


def required():
    it = ["src:n=%d" % n for n in (1, 2, 3)] + ["src:c0%4==0,c0!=0", "src:c0%4!=0"] + ["src:cn%%4=%d" % r for r in (1, 2, 3)]
    it += ["src:cn%4!=0-before-another-source", "src:slice-ends-at-unpadded-row-end", "src:input-slice", "src:input-by-later-op",
           "src:input+op-concat", "src:three-consumers", "src:same-tensor-twice"]
    it += ["dag:diamond-max-not-last-consumer", "dag:diamond-max-not-first-consumer", "dag:unread-middle", "dag:chain48", "dag:one-op",
           "dag:k1-only", "head:tf=1", "head:tf>256", "dag:in_reach>256"]
    it += ["ring:R>256-kernel", "ring:R>256-dilation-k2", "ring:R>call", "ring:three-unequal-sources", "call:one-output-chain"]
    it += ["width:cout%%4=%d" % r for r in (1, 2, 3)] + ["width:cout=1", "width:cout=1024", "width:cin=1", "bn:groups=1", "bn:groups=2",
                                                        "bn:groups=3", "bn:groups=cout", "width:c_last%4!=0"]
    it += ["limit:kernel=1024", "limit:dilation=1024", "limit:filters=1024", "limit:n_ops=48", "limit:final-map>=2^18"]
    it += ["arena:reuse-float", "arena:reuse-bytes", "arena:plans-reuse-differently", "arena:flags-differ", "sync:0-shared-interval",
           "sync:1-out-read-only"]
    it += ["tile:lds<64K", "tile:lds-64K-160K", "tile:lds-largest", "tile:scratch-smallest"]
    it += ["call:outputs=%d" % n for n in (255, 256, 257, 513)]
    it += ["call:tiles>2CU", "call:zero-output-between", "call:empty-track-first", "call:empty-track-middle", "call:empty-track-last",
           "call:padded-tracks", "call:frames-u16", "call:frames-f32", "call:frames-host", "call:reset-between", "call:two-streams"]
    it += ["ns:track=T", "ns:track=T-1", "ns:track=0", "ns:>256-windows-behind-short", "ns:drop!=0", "ns:drop-beyond-alignment"]
    return it + list(BRANCH_ITEMS) + list(UNREACHABLE)


def items_of(c, with_oracle=True):
    """the items a case covers, computed from its description, its script, the restated plan and (the requantization branches)
    the oracle"""
    d, pl = c.desc, Plan(c.desc)
    ops, n = d["conv_ops"], pl.n
    it = set()
    readers = {t: [] for t in range(-1, n)}
    for i in range(n):
        srcs = pl.src[i]
        it.add("src:n=%d" % len(srcs))
        for j, (s, c0, cn, sch) in enumerate(srcs):
            readers[s].append(i)
            if c0 and c0 % 4 == 0:
                it.add("src:c0%4==0,c0!=0")
            if c0 % 4:
                it.add("src:c0%4!=0")
            if cn % 4:
                it.add("src:cn%%4=%d" % (cn % 4))
                if j + 1 < len(srcs):
                    it.add("src:cn%4!=0-before-another-source")
            if sch % 4 and c0 + cn == sch and (c0 or cn != sch):
                it.add("src:slice-ends-at-unpadded-row-end")
            if s < 0 and (c0, cn) != (0, BINS):
                it.add("src:input-slice")
            if s < 0 and i > 0:
                it.add("src:input-by-later-op")
        if any(s < 0 for s, _, _, _ in srcs) and any(s >= 0 for s, _, _, _ in srcs):
            it.add("src:input+op-concat")
        tens = [s for s, _, _, _ in srcs]
        if len(set(tens)) < len(tens):
            it.add("src:same-tensor-twice")
        if len(srcs) == 3 and len({cn for _, _, cn, _ in srcs}) == 3 and pl.R[i]:
            it.add("ring:three-unequal-sources")
        k, dil, f, g = pl.k[i], int(ops[i].get("dilation", 1)), pl.cout[i], int(ops[i].get("bn_groups", 1))
        if f % 4:
            it.add("width:cout%%4=%d" % (f % 4))
        if f in (1, 1024):
            it.add("width:cout=%d" % f)
        if pl.cin[i] == 1:
            it.add("width:cin=1")
        for name, hit in (("bn:groups=1", g == 1), ("bn:groups=2", g == 2), ("bn:groups=3", g == 3), ("bn:groups=cout", g == f and f > 3),
                          ("limit:kernel=1024", k == 1024), ("limit:dilation=1024", dil == 1024), ("limit:filters=1024", f == 1024),
                          ("ring:R>256-kernel", pl.R[i] > TILE and dil == 1), ("ring:R>256-dilation-k2", pl.R[i] > TILE and k == 2),
                          ("dag:unread-middle", pl.last_use[i] < 0 and 0 < i < n - 1)):
            if hit:
                it.add(name)
    for t in range(-1, n):
        if len(set(readers[t])) >= 3:
            it.add("src:three-consumers")
        asked = pl.asked[t]   # in the order the planner meets them: the latest consumer first
        if len({i for i, _ in asked}) >= 2:
            top = max(w for _, w in asked)
            if asked[0][1] < top:
                it.add("dag:diamond-max-not-last-consumer")
            if asked[-1][1] < top:
                it.add("dag:diamond-max-not-first-consumer")
    for name, hit in (("dag:chain48", n == 48 and all(pl.src[i][0][0] == i - 1 and len(pl.src[i]) == 1 for i in range(n))), ("dag:one-op", n == 1),
                      ("limit:n_ops=48", n == 48), ("dag:k1-only", n > 1 and not any(pl.R) and pl.n_state == (pl.tf - 1) * pl.c_last),
                      ("head:tf=1", pl.tf == 1), ("head:tf>256", pl.tf > TILE), ("dag:in_reach>256", pl.in_reach > TILE),
                      ("width:c_last%4!=0", pl.c_last % 4), ("limit:final-map>=2^18", pl.tf * pl.c_last >= 1 << 18)):
        if hit:
            it.add(name)
    # the arena and the barrier rule, from the restated plan
    f32, q8 = pl.f32, pl.q8
    for name, hit in (("arena:reuse-float", any(f32.reused)), ("arena:reuse-bytes", any(q8.reused)),
                      ("arena:plans-reuse-differently", f32.reused != q8.reused), ("arena:flags-differ", f32.sync != q8.sync),
                      ("sync:0-shared-interval", any(not s for p in (f32, q8) for s in p.sync[1:])),
                      ("sync:1-out-read-only", any(w == (True, False, False) for p in (f32, q8) for w in p.why))):
        if hit:
            it.add(name)
    if tile_placement(pl) != "scratch":
        it.add("tile:" + tile_placement(pl))
    # the two tiles next to the limit: one pitch step (4 channels of the largest tensor) changes the placement
    if pl.tile_bytes <= KMAX_LDS < (_tile_bytes(_widened(d, 4)) or 0):
        it.add("tile:lds-largest")
    if pl.tile_bytes > KMAX_LDS >= (_tile_bytes(_widened(d, -4)) or KMAX_LDS + 1):
        it.add("tile:scratch-smallest")
    # stream-mode script
    since_reset_ones, had_output = True, False
    longest = max(pl.R + [pl.tf - 1])
    for i, st in enumerate(c.script):
        n_out = 0
        if st[0] == "tracks":
            lens, pads = st[1], st[2]
            n_out = sum(lens)
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
            n_out = 1 if st[0] == "ones" else (10 ** 6 if st[1] == "grid" else st[1])
        if st[0] == "outputs":
            if st[1] == "grid":
                it.add("call:tiles>2CU")
            elif st[1] in (255, 256, 257, 513):
                it.add("call:outputs=%d" % st[1])
        if had_output and 0 < n_out < max(pl.R + [0]):
            it.add("ring:R>call")   # the ring shifts by the call's frames: part of it survives the call
        if st[0] == "ones":
            if since_reset_ones and st[1] >= longest + 2 and longest > 0:
                it.add("call:one-output-chain")
        elif st[0] == "reset":
            since_reset_ones, had_output = True, False
            if 0 < i < len(c.script) - 1:
                it.add("call:reset-between")
        elif st[0] != "zero":
            since_reset_ones = False
        had_output = had_output or n_out > 0
        if st[0] == "zero" and 0 < i < len(c.script) - 1 and c.script[i - 1][0] != "reset" and c.script[i + 1][0] != "reset":
            it.add("call:zero-output-between")
    if c.two:
        it.add("call:two-streams")
    # non-stream twin
    T, lens = d["frames"], c.ns[0]
    for name, v in (("ns:track=T", T), ("ns:track=T-1", T - 1), ("ns:track=0", 0)):
        if v in lens:
            it.add(name)
    if lens and lens[-1] - T + 1 > TILE and any(0 < v < T + 4 for v in lens[:-1]):
        it.add("ns:>256-windows-behind-short")
    if any(any(o["drop"]) for o in ops):
        it.add("ns:drop!=0")
    if any(min(o["drop"]) > 0 for o in ops):
        it.add("ns:drop-beyond-alignment")
    if with_oracle:
        it |= set(oracle_report(c.id)[1]) & set(BRANCH_ITEMS)
    return it


def uncovered(case_list=None):
    have = set()
    for c in (case_list if case_list is not None else _cases()):
        have |= items_of(c)
    return [i for i in required() if i not in have]


def describe(c):
    pl = Plan(c.desc)
    ops = ["%s%s k%d d%d f%d g%d" % ([s for s, _, _, _ in pl.src[i]], [(c0, cn) for _, c0, cn, _ in pl.src[i]], pl.k[i],
                                      int(o.get("dilation", 1)), pl.cout[i], int(o.get("bn_groups", 1))) for i, o in enumerate(c.desc["conv_ops"])]
    return "%s: %d ops %s, t_final %d, window %d, in_reach %d, state %d, float sync %s, byte sync %s, int8 tile %d B (%s), items %s" % (
        c.id, pl.n, ops if pl.n <= 8 else ops[:4] + ["..."], pl.tf, c.desc["frames"], pl.in_reach, pl.n_state, "".join(map(str, pl.f32.sync)),
        "".join(map(str, pl.q8.sync)), pl.tile_bytes, tile_placement(pl), sorted(items_of(c, with_oracle=False)))


def cost(c):
    """a rough count of multiply-adds of one pass over the script (cheapest cases first in the emulator slice): every call
    recomputes each tensor's reach in front of every tile"""
    pl = Plan(c.desc)

    def call(n):
        if not n:
            return 0
        tiles = -(-n // TILE)
        return sum((n + tiles * pl.reach[i]) * pl.k[i] * pl.cin[i] * pl.cout[i] for i in range(pl.n)) + n * pl.tf * pl.c_last

    total = 0
    for st in c.script:
        total += {"tracks": lambda: call(sum(st[1])), "host": lambda: call(st[1]), "ones": lambda: st[1] * call(1),
                  "outputs": lambda: call(2500 if st[1] == "grid" else st[1])}.get(st[0], lambda: 0)()
    return (2 if c.two else 1) * total + 12 * call(c.cap)


def emulator_slice():
    """every item once, cheapest cases first (greedy): the part of the plan the CPU suite runs through the emulated kernels"""
    need, out = set(required()) - set(UNREACHABLE), []
    for c in sorted(_cases(), key=cost):
        got = items_of(c) & need
        if got:
            out.append(c)
            need -= got
    assert not need, need
    return out


# ------------------------------------------------------------------------------------------------------ running
def _finite(a, what):
    assert np.all(np.isfinite(a)), what + ": the engine returned a NaN or an infinity"


def compare_state(got, ref, net, what):
    """``mww_stream_get_state`` against the oracle's rings: a ring fed by the spectrogram alone is a copy of input frames
    (bit-equal), every other ring holds activations (FWD_TOL).  Returns the largest activation-ring error."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    _finite(got, what)
    at, worst = 0, 0.0
    for name, rows, ch, raw in net.ring_shapes():
        g, r = got[at:at + rows * ch], ref[at:at + rows * ch]
        if raw:
            assert np.array_equal(g, r.astype(np.float32)), (what, "ring of op %s (input frames) differs" % name)
        else:
            e = float(np.abs(g - r).max())
            assert e <= ec.FWD_TOL, (what, "ring of %s" % name, e)
            worst = max(worst, e)
        at += rows * ch
    assert at == got.size
    return worst


class _Session:
    """one stream (float or int8) of a case driven through the script, every call held to the oracle"""

    def __init__(self, lib, b, kind, seed, n_cu, stores, worst):
        from microwakeword_amd import native, streaming
        self.b, self.kind, self.seed, self.n_cu, self.stores, self.worst = b, kind, seed, n_cu, stores, worst
        self.model = sc.context_model(lib)
        if kind == "float":
            self.st = native.GraphStream(self.model.engine, b.desc)
            self.st.set_weights(b.flat)
        else:
            self.qsm = streaming.QuantizedStreamingModel(b.qm, 1, "stream", context=self.model)
            self.st = self.qsm.native
        self._reset_oracle()

    def _reset_oracle(self):
        self.fed, self.only_ones = [], True
        self.step = sgo.StepStream(self.b.net) if self.kind == "float" else qgo.StepStreamQ8(self.b.qm)

    def _state(self):
        return self.st.get_state() if self.kind == "float" else self.st.get_state_q8()

    def _check(self, n_new, what, step_ref=None):
        """the last call's n_new outputs and the state against the oracle over everything fed since the reset"""
        b = self.b
        fed = np.concatenate(self.fed + [np.zeros((0, BINS), np.float32)], 0)
        if self.kind == "float":
            p, z = self.st.read(want_logits=True)
            assert p.size == n_new, (what, p.size, n_new)
            _finite(p, what)
            _finite(z, what)
            if step_ref is not None:
                ref_z, ref_st = step_ref
            else:
                ref_z, ref_st = sgo.whole_sequence(b.net, fed, rings=True)
                ref_z = ref_z[ref_z.size - n_new:]
            sc._compare(p, z, ref_z, what)
            if n_new:
                self.worst["logit"] = max(self.worst["logit"], float(np.abs(z - ref_z).max()))
                self.worst["prob"] = max(self.worst["prob"], float(np.abs(p - sgo.sigmoid(ref_z)).max()))
            self.worst["state"] = max(self.worst["state"], compare_state(self._state(), ref_st, b.net, what))
        else:
            u8 = self.st.read_q8()
            assert u8.size == n_new, (what, u8.size, n_new)
            if step_ref is not None:
                ref_lq, ref_st = step_ref
                ref_u8 = b.qm.lut[np.asarray(ref_lq, np.int64) + 128]
            else:
                ref_u8, ref_lq, ref_st = qgo.whole_sequence(b.qm, fed)
                ref_u8, ref_lq = ref_u8[ref_u8.size - n_new:], ref_lq[ref_lq.size - n_new:]
            lq = self.st.read(want_logits=True)[1]
            assert np.array_equal(u8, ref_u8), "%s: %d of %d uint8 outputs differ (%d int8 logits)" % (
                what, int(np.sum(u8 != ref_u8)), u8.size, int(np.sum(lq != np.asarray(ref_lq, np.float32))))
            qc.check_logits(self.qsm, ref_lq, what)
            got_st = self._state()
            assert np.array_equal(got_st, ref_st), "%s: rings differ at %s" % (what, np.nonzero(got_st != ref_st)[0][:8])
            qgc._check_probs(self.qsm, u8)

    def run(self, i):
        b = self.b
        st = b.case.script[i]
        what = "%s %s step %d %s" % (b.case.id, self.kind, i, st[0])
        rng = _rng(b.case.id, self.seed, i)
        if st[0] == "reset":
            self.st.reset()
            self._reset_oracle()
        elif st[0] == "zero":
            before = self._state()
            n = self.st.run_host(np.zeros((0, BINS), np.float32))
            assert n == 0 and self.st.n_out == 0, what
            assert np.array_equal(before.view(np.uint8), self._state().view(np.uint8)), what + ": a call without outputs changed the state"
        elif st[0] == "tracks":
            tr = sc.Tracks(self.model, st[1], st[2], seed=int(rng.integers(1 << 30)), store_ids=self.stores)
            off = self.st.run(tr.win)
            assert list(np.diff(off)) == list(st[1]), (what, "offsets", off)
            self.fed += tr.frames
            self.only_ones = False
            self._check(int(off[-1]), what)
        elif st[0] in ("host", "outputs"):
            L = st[1] if st[0] == "host" else ((2 * self.n_cu + 2) * TILE + 5 if st[1] == "grid" else st[1])
            x = gen_frames(rng, L, "u16" if i % 2 else "f32")
            n = self.st.run_host(x)
            assert n == L, what
            self.fed.append(x)
            self.only_ones = False
            self._check(n, what)
        elif st[0] == "ones":
            for j in range(st[1]):
                x = gen_frames(rng, 1)
                assert self.st.run_host(x) == 1, what
                self.fed.append(x)
                ref = None
                if self.only_ones:   # the literal ring form, one step per call
                    lz = self.step.step(x)
                    ref = (np.array([lz]), self.step.state())
                self._check(1, "%s call %d" % (what, j), ref)
        else:
            raise ValueError(st)

    def close(self):
        self.st.close()


def _chunking(lib, b, kind):
    """any split of the sequence into calls gives bit for bit the probabilities and the final state of one call; a second
    run of the one call does too"""
    from microwakeword_amd import native, streaming
    model = sc.context_model(lib)

    def fresh():
        if kind == "float":
            st = native.GraphStream(model.engine, b.desc)
            st.set_weights(b.flat)
            return st
        return streaming.QuantizedStreamingModel(b.qm, 1, "stream", context=model).native

    def state(st):
        return (st.get_state() if kind == "float" else st.get_state_q8()).view(np.uint8)

    n_out = len(b.seq)
    st = fresh()
    assert st.run_host(b.seq) == n_out
    p0, z0 = st.read(want_logits=True)
    s0 = state(st)
    st.close()
    st = fresh()   # two-run bit equality
    st.run_host(b.seq)
    assert np.array_equal(st.read().view(np.uint32), p0.view(np.uint32)) and np.array_equal(state(st), s0), b.case.id + ": reruns differ"
    st.close()
    for si, pieces in enumerate(ss._splits(_rng(b.case.id, 77), n_out, 1)):
        st = fresh()
        ps = []
        for lo, hi in pieces:
            assert st.run_host(b.seq[lo:hi]) == hi - lo
            ps.append(st.read())
        assert np.array_equal(np.concatenate(ps).view(np.uint32), p0.view(np.uint32)), "%s %s split %d %s: probabilities differ" % (
            b.case.id, kind, si, pieces)
        assert np.array_equal(state(st), s0), "%s %s split %d %s: final state differs" % (b.case.id, kind, si, pieces)
        st.close()
    return p0, z0, s0


def _rec(lib, b, p0, z0, s0, worst):
    """the REC form (``calibrate_host`` on a stream created with int8=True) on the case's sequence: every tensor's recorded
    (min, max) - those of ops nobody reads too - against ``quant_graph_checks.desc_ranges`` within RANGE_RTOL, and the float
    outputs and state unchanged"""
    from microwakeword_amd import native
    model = sc.context_model(lib)
    st = native.GraphStream(model.engine, b.desc, int8=True)
    st.set_weights(b.flat)
    ranges = st.calibrate_host(b.seq)
    assert ranges.shape == (len(b.desc["conv_ops"]) + 2, 2)
    _finite(ranges, b.case.id + " REC")
    assert np.array_equal(st.read().view(np.uint32), p0.view(np.uint32)), b.case.id + ": REC changes the probabilities"
    assert np.array_equal(st.get_state().view(np.uint8), s0), b.case.id + ": REC changes the state"
    st.close()
    assert ranges[-1, 0] == z0.min() and ranges[-1, 1] == z0.max()
    assert ranges[0, 0] == b.seq.min() and ranges[0, 1] == b.seq.max()
    ref = qgc.desc_ranges(b.desc, b.weights, b.seq)
    for t, (got, want) in enumerate(zip(ranges.astype(np.float64), ref)):
        mag = max(abs(want[0]), abs(want[1]), 1e-30)
        worst["range"] = max(worst["range"], float(np.abs(got - want).max() / (qgc.RANGE_RTOL * mag)))
        assert np.all(np.abs(got - want) <= qgc.RANGE_RTOL * mag), (b.case.id, "range of tensor %d" % t, got, want)


def _non_stream(lib, b, kinds, worst):
    from microwakeword_amd import native, streaming
    model = sc.context_model(lib)
    lens, pads = b.case.ns
    tr = sc.Tracks(model, lens, pads, seed=SEED)
    want = [max(0, L - b.T + 1) for L in lens]
    if "float" in kinds:
        st = native.GraphStream(model.engine, dict(b.desc, mode="non_stream"))
        st.set_weights(b.flat)
        off = st.run(tr.win)
        assert list(np.diff(off)) == want, (b.case.id, "non_stream offsets", off)
        p, z = st.read(want_logits=True)
        _finite(z, b.case.id + " non_stream")
        for t, f in enumerate(tr.frames):
            ref = sgo.non_stream_windows(b.net, f.astype(np.float64), b.T)
            sc._compare(p[off[t]:off[t + 1]], z[off[t]:off[t + 1]], ref, "%s non_stream track %d" % (b.case.id, t))
            if ref.size:
                worst["logit"] = max(worst["logit"], float(np.abs(z[off[t]:off[t + 1]] - ref).max()))
        st.close()
    if "q8" in kinds:
        qsm = streaming.QuantizedStreamingModel(b.qm, 1, "non_stream", context=model)
        off = qsm.native.run(tr.win)
        assert list(np.diff(off)) == want, (b.case.id, "int8 non_stream offsets", off)
        u8, lq = qsm.read_q8(), []
        for t, f in enumerate(tr.frames):
            ref_u8, ref_lq = qgo.non_stream(b.qm, f, b.T, want_logits=True)
            assert np.array_equal(u8[off[t]:off[t + 1]], ref_u8), "%s int8 non_stream track %d" % (b.case.id, t)
            lq.append(ref_lq)
        qc.check_logits(qsm, np.concatenate(lq + [np.zeros(0, np.int8)]), b.case.id + " int8 non_stream")
        qgc._check_probs(qsm, u8)
        qsm.native.close()


def run_case(lib, c, n_cu=256, kinds=("float", "rec", "q8")):
    """one case through the float kernel, its REC form and the int8 kernel; returns the figures of the results file"""
    b = built(c.id)
    t0 = time.time()
    worst = {"logit": 0.0, "prob": 0.0, "state": 0.0, "range": 0.0}
    if "q8" in kinds and c.spread:
        qgc.check_spread(b.qm, b.seq, c.id)   # a condition on the inputs: before any kernel runs
    for kind in kinds:
        if kind == "rec":
            continue
        sessions = [_Session(lib, b, kind, 0, n_cu, (0, 1), worst)] + ([_Session(lib, b, kind, 1, n_cu, (2, 3), worst)] if c.two else [])
        for i in range(len(c.script)):
            for ses in sessions:   # two streams of one context, alternately: independent rings
                ses.run(i)
        for ses in sessions:
            ses.close()
        p0, z0, s0 = _chunking(lib, b, kind)
        if kind == "float" and "rec" in kinds:
            _rec(lib, b, p0, z0, s0, worst)
    _non_stream(lib, b, kinds, worst)
    return dict(id=c.id, seconds=round(time.time() - t0, 2), logit_ratio=worst["logit"] / ec.FWD_TOL, prob_ratio=worst["prob"] / sc.PROB_TOL,
                state_ratio=worst["state"] / ec.FWD_TOL, rec_range_ratio=worst["range"], condition=[round(v, 4) for v in float32_condition(c.id)],
                branches=sorted(oracle_report(c.id)[1]))
