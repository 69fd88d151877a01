"""Checks of the streaming evaluation of MixedNets with residual connections, a pooled head or spatial attention
(``mww_stream_create_mixednet``, stream_forward_kernel<true, *> of csrc/tu_stream.hip) shared by the emulator tests
(tests/test_mixednet_variant_emulated.py) and the GPU tests (tests/test_mixednet_variant_gpu.py), in the manner of
tests/stream_sweep.py:

- ``cases()`` is a hand-written list of small cases (widths of at most 16 channels).  A case is an extended stream description
  (``native.Stream``: residual / attention / pool next to the usual keys), Keras-order weights for it (``OracleModel`` of the
  equivalent flag set, BatchNorm statistics from a float64 dry run), a stream-mode call script and a non_stream twin.  What
  a case covers is COMPUTED from its description and script (``items_of``); ``uncovered()`` must come back empty.
- ``float32_condition`` is a condition on a case's INPUTS computed from the oracles alone: the float32 run of the
  restatement stays within a quarter of each bound of the float64 one (the CPU test asserts it for every case).
- ``run_case(lib, case, n_cu)`` drives one case through the kernel and holds every call to the float64 oracles
  (tests/mixednet_variant_streaming_oracle.py, ``OracleModel`` for the non_stream windows): outputs, logits AND rings.
  A spatial-attention case has no stream mode (refused): its checks are the non_stream twin and the rerun.
"""
import functools
import time

import numpy as np
import torch

import engine_checks as ec
import mixednet_variant_streaming_oracle as vo
import stream_sweep as sw
import streaming_checks as sc
import streaming_oracle as so
from oracle import model_oracle as mo

SEED = 2027
TILE = sw.TILE
CHAIN_MAX_RING = 40


# ------------------------------------------------------------------------------------------------- descriptions
def desc_of(c1, k1, s, blocks, tf, residual=None, attention=0, pool=0, frames=None):
    """blocks: [(repeat, kernel sizes, filters)]; tf: frames of the final map before attention and pooling"""
    d = sw.desc_of(c1, k1, s, blocks, tf, frames)
    d.update(residual=list(residual) if residual is not None else [0] * len(blocks), attention=attention, pool=pool)
    return d


def flags_of(desc):
    """the MixedNet flag set of an extended description.  ``pool`` stays in the flags when t_final is 1: there the reference
    ignores it and so must everything here"""
    return dict(sc.flags_of(desc), residual_connection="".join("%d," % r for r in desc["residual"]),
                spatial_attention=int(desc["attention"]), pooled=int(bool(desc["pool"])), max_pool=int(desc["pool"] == "max"))


class Case:
    """``script`` / ``ns``: as tests/stream_sweep.py Case (stream-mode steps on one stream; lengths and pads of the
    non_stream twin).  ``bn_shift`` / ``dense_scale``: scalings of the random weights named in the id when not 0 / 1."""

    def __init__(self, cid, desc, script=None, ns=None, cap=700, bn_shift=0.0, dense_scale=1.0):
        self.id, self.desc = cid, desc
        s, T = desc["stride"], desc["frames"]
        chain = max(sw.ring_lengths(desc)) + 2
        self.script = script if script is not None else [
            ("tracks", [0, 7, T + 5, 0, 3, 2 * T + s + 1, 0], [0, 2, 0, 0, 0, 4, 0]),
            ("zero",),
            ("host", T + 9),
            ("reset",),
            ("ones", chain if chain - 2 <= CHAIN_MAX_RING else 3),
            ("tracks", [300 * s + 1, 2], [0, 0]),
        ]
        if desc["attention"]:
            self.script = []
        self.ns = ns if ns is not None else ([T, T - 1, 0, T + s - 1, T + 3 * s + 1], [T // 2, 0, 0, 0, 0])
        self.bn_shift, self.dense_scale, self.cap = bn_shift, dense_scale, cap

    def __repr__(self):
        return self.id


def cases():
    out = []
    # residual on the first and the last block, both with Cin != F; repeat 2; stride 2 with k1 > s; the residual blocks'
    # width 8 is cmax
    out.append(Case("res-first-last_cin-ne-f_rep2_s2-k1gt_tf3",
                    desc_of(6, 5, 2, [(2, (3,), 8), (1, (3, 5), 8), (1, (3,), 5)], 3, residual=[1, 0, 1])))
    # three consecutive residual blocks: Cin == F with repeat 3; a block without a depthwise layer; two MixConv groups;
    # k1 == s; average pooling over T_f = 2
    out.append(Case("res-consecutive_cin-eq-f_rep3_nodw_g2_s1-k1eq_avg-tf2",
                    desc_of(8, 1, 1, [(3, (3,), 8), (1, (1,), 12), (1, (3, 5), 7)], 2, residual=[1, 1, 1], pool="average")))
    # stride 3 with k1 < s; max pooling over T_f = 5; residual on the first block only
    out.append(Case("res-first_s3-k1lt_max-tf5", desc_of(5, 2, 3, [(1, (3,), 6), (1, (5,), 9)], 5, residual=[1, 0], pool="max")))
    # exact tile boundaries and more tiles than 2 x CU workgroups, a non_stream track of more than 256 windows: average
    # pooling over T_f = 5 behind a residual block, tiny widths
    out.append(Case("tile-edges_grid_avg-tf5_res", desc_of(4, 3, 1, [(1, (3,), 6)], 5, residual=[1], pool="average"),
                    script=[("outputs", 255), ("outputs", 256), ("zero",), ("outputs", 257), ("outputs", 513), ("outputs", "grid"),
                            ("reset",), ("ones", 7), ("outputs", 256)],
                    ns=([13, 9, 11, 0, 262 + 9], [0, 0, 2, 0, 0])))
    # max pooling over T_f = 2, Cin == F
    out.append(Case("max-tf2_res", desc_of(4, 3, 1, [(1, (3,), 4)], 2, residual=[1], pool="max")))
    # a pooled head over more frames than a tile has outputs: the head ring is longer than a tile
    out.append(Case("avg-tf300_res", desc_of(4, 3, 1, [(1, (3,), 6)], 300, residual=[1], pool="average"),
                    script=[("tracks", [0, 100, 320, 0], [0, 5, 0, 0]), ("zero",), ("outputs", 257), ("reset",), ("ones", 4),
                            ("outputs", 330)], cap=900))
    # the pooled flags with T_f = 1 do nothing: the plain model, on the plain kernel
    out.append(Case("pooled-flags_tf1_plain", desc_of(5, 3, 1, [(1, (3,), 7)], 1, pool="max")))
    # spatial attention (non_stream only): T_f = 4 and 5, with and without pooling, one behind a residual block
    out.append(Case("att-tf4", desc_of(6, 3, 1, [(1, (3,), 8)], 4, attention=1)))
    out.append(Case("att-tf5_res_s2", desc_of(6, 3, 2, [(1, (3,), 8), (2, (3, 5), 6)], 5, residual=[0, 1], attention=1)))
    out.append(Case("att-tf4_avg", desc_of(5, 3, 1, [(1, (5,), 7)], 4, attention=1, pool="average")))
    out.append(Case("att-tf5_max_res", desc_of(5, 3, 1, [(1, (5,), 7)], 5, residual=[1], attention=1, pool="max"),
                    ns=([11, 10, 0, 11 + 300], [3, 0, 0, 0])))
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


# ------------------------------------------------------------------------------------------------------- items
def required():
    it = ["res:cin!=f", "res:cin==f", "res:first-block", "res:last-block", "res:consecutive", "res:repeat=2", "res:repeat=3",
          "res:no-depthwise", "res:multi-group", "res:width=cmax"]
    it += ["conv1:s=%d" % s for s in (1, 2, 3)] + ["conv1:k1>s", "conv1:k1==s", "conv1:k1<s"]
    it += ["call:outputs=%d" % n for n in (255, 256, 257, 513)] + ["call:tiles>2CU", "ns:>256-windows"]
    it += ["call:frames-u16", "call:frames-f32", "call:frames-host", "call:padded-tracks", "call:empty-track", "call:one-output-chain",
           "call:reset-between"]
    it += ["pool:avg-tf=2", "pool:avg-tf=5", "pool:max-tf=2", "pool:max-tf=5", "pool:tf>256", "pool:flags-with-tf=1"]
    it += ["att:tf=4", "att:tf=5", "att:tf=4+pool", "att:tf=5+pool"]
    return it


def items_of(c):
    """the items a case covers, computed from its description and its script"""
    d = c.desc
    k1, s, tf = d["conv1_kernel"], d["stride"], d["t_final"]
    it = {"conv1:s=%d" % s, "conv1:k1>s" if k1 > s else ("conv1:k1==s" if k1 == s else "conv1:k1<s")}
    cm, cin, nb = sw.cmax_of(d), d["conv1_filters"], len(d["blocks"])
    for bi, ((rep, ks, f), r) in enumerate(zip(d["blocks"], d["residual"])):
        if r:
            it.add("res:cin==f" if cin == f else "res:cin!=f")
            if bi == 0:
                it.add("res:first-block")
            if bi == nb - 1:
                it.add("res:last-block")
            if bi and d["residual"][bi - 1]:
                it.add("res:consecutive")
            if rep in (2, 3):
                it.add("res:repeat=%d" % rep)
            if max(ks) == 1:
                it.add("res:no-depthwise")
            elif len(ks) > 1:
                it.add("res:multi-group")
            if f == cm:
                it.add("res:width=cmax")
        cin = f
    pool, att = d["pool"], d["attention"]
    if att:
        it.add("att:tf=%d%s" % (tf, "+pool" if pool else ""))
    elif pool and tf == 1:
        it.add("pool:flags-with-tf=1")
    elif pool:
        it.add("pool:%s-tf=%d" % ("avg" if pool == "average" else "max", tf))
        if tf > TILE:
            it.add("pool:tf>256")
    since_reset_ones = True
    for i, st in enumerate(c.script):
        if st[0] == "tracks":
            it.update({"call:frames-u16"} | ({"call:frames-f32"} if len(st[1]) > 1 else set()))
            if any(v == 0 for v in st[1]):
                it.add("call:empty-track")
            if any(st[2]):
                it.add("call:padded-tracks")
        if st[0] in ("host", "outputs", "ones"):
            it.add("call:frames-host")
        if st[0] == "outputs":
            it.add("call:tiles>2CU" if st[1] == "grid" else "call:outputs=%d" % st[1])
        if st[0] == "ones":
            if since_reset_ones and st[1] >= max(sw.ring_lengths(d)) + 2:
                it.add("call:one-output-chain")
        elif st[0] == "reset":
            since_reset_ones = True
            if 0 < i < len(c.script) - 1:
                it.add("call:reset-between")
        elif st[0] != "zero":
            since_reset_ones = False
    T = d["frames"]
    if any((L - T) // s + 1 > TILE for L in c.ns[0] if L >= T):
        it.add("ns:>256-windows")
    return it


def uncovered(case_list=None):
    have = set()
    for c in (case_list if case_list is not None else _cases()):
        have |= items_of(c)
    return [i for i in required() if i not in have]


# ------------------------------------------------------------------------------------------- weights and frames
class Built:
    pass


def _condition_bn(flags, om, T, frames, shift=0.0):
    """BatchNorm moving statistics := the statistics of each 1x1 layer's output (a block's residual 1x1 included) on a
    float64 dry run of the streaming body, as stream_sweep._condition_bn"""
    names = [v.name for v in om.vars]
    w = om.get_weights()

    def set_bn(prefix, y):
        var = y.var(axis=0)
        w[names.index(prefix + ".moving_mean")] = (y.mean(axis=0) - shift * np.sqrt(var)).astype(np.float32)
        w[names.index(prefix + ".moving_variance")] = np.where(var > 1e-12, var, 1.0).astype(np.float32)
        om.set_weights(w)
        return vo.Net(flags, om, T, body_only=True)

    net = vo.Net(flags, om, T, body_only=True)
    a = net.conv1(np.concatenate([np.zeros((net.r1, 40)), np.asarray(frames, np.float64)], 0))
    r = {}
    for kind, p, ks in net.layers:
        if kind == "res":
            net = set_bn(p + ".res.bn", a @ net.w[p + ".res.kernel"][0, 0])
            r[p] = net.res(p, a)
        elif kind == "mix":
            a = net.mix(p, ks, np.concatenate([np.zeros((max(ks) - 1, a.shape[1])), a], 0))
        else:
            net = set_bn(p + ".bn", a @ net.w[p + ".pw.kernel"][0, 0])
            a = net.pw_res(p, a, r[ks] if ks else None)
    return om


@functools.lru_cache(maxsize=None)
def built(cid):
    c = case(cid)
    b = Built()
    b.case, b.desc = c, c.desc
    b.flags = flags_of(c.desc)
    b.T, b.s = c.desc["frames"], c.desc["stride"]
    om = ec.perturbed_oracle(b.T, seed=SEED, flags=b.flags)
    assert vo.t_final_of(b.flags, b.T) == c.desc["t_final"], cid
    if c.dense_scale != 1.0:
        om.set_weights([w * np.float32(c.dense_scale) if v.name.startswith("dense.") else w for v, w in zip(om.vars, om.get_weights())])
    b.seq = sw.gen_frames(sw._rng(cid, 0), c.cap * b.s, "u16")
    b.om = _condition_bn(b.flags, om, b.T, b.seq, c.bn_shift)
    b.net = None if c.desc["attention"] else vo.Net(b.flags, b.om, b.T)
    b.weights = b.om.get_weights()
    b.flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in b.weights])
    return b


def ns_tracks(b):
    """the frames of the non_stream twin's tracks, as sc.Tracks(model, lens, pads, seed=SEED) generates them"""
    rng = np.random.default_rng(SEED)
    out = []
    for i, (L, pad) in enumerate(zip(*b.case.ns)):
        rows = L - pad
        if i % 2 == 0:
            x = rng.integers(0, 1200, size=(rows, 40)).astype(np.uint16).astype(np.float32) * np.float32(0.0390625)
        else:
            x = rng.uniform(0, 40, size=(rows, 40)).astype(np.float32)
        out.append(np.concatenate([np.zeros((pad, 40), np.float32), x], 0))
    return out


def float32_condition(cid):
    """the float32 run of the restatement against the float64 one, as fractions of the bounds: (logits / FWD_TOL,
    probabilities / PROB_TOL, activation rings / FWD_TOL) - stream mode over the case's sequence through
    mixednet_variant_streaming_oracle, and the non_stream windows of the twin's tracks through OracleModel in float32
    (the only form a spatial-attention case has).  The CPU test asserts each <= 1/4 for every case."""
    b = built(cid)
    zr = pr = sr = 0.0
    if b.net is not None:
        z64, st64 = vo.whole_sequence(b.net, b.seq, rings=True)
        z32, st32 = vo.whole_sequence(vo.Net(b.flags, b.om, b.T, dtype=np.float32), b.seq, rings=True)
        n1 = b.net.r1 * 40
        zr = float(np.abs(z32 - z64).max()) / ec.FWD_TOL
        pr = float(np.abs(so.sigmoid(z32) - so.sigmoid(z64)).max()) / sc.PROB_TOL
        sr = (float(np.abs(st32[n1:] - st64[n1:]).max()) if st64.size > n1 else 0.0) / ec.FWD_TOL
    om32 = mo.OracleModel("mixednet", b.flags, b.T, seed=SEED, dtype=torch.float32)
    om32.set_weights(b.weights)
    for f in ns_tracks(b):
        if len(f) >= b.T:
            x = np.stack([f[e - b.T:e] for e in range(b.T, len(f) + 1, b.s)])
            z64, z32 = b.om.predict_with_logits(x.astype(np.float64))[1], np.asarray(om32.predict_with_logits(x)[1], np.float64)
            zr = max(zr, float(np.abs(z32 - z64).max()) / ec.FWD_TOL)
            pr = max(pr, float(np.abs(so.sigmoid(z32) - so.sigmoid(z64)).max()) / sc.PROB_TOL)
    return zr, pr, sr


# ------------------------------------------------------------------------------------------------------ running
def new_stream(lib, b, mode="stream"):
    from microwakeword_amd import native
    st = native.Stream(sc.context_model(lib).engine, dict(b.desc, mode=mode))
    st.set_weights(b.flat)
    return st


class _Session:
    """one stream of a case driven through the script, every call held to the oracle: outputs, logits and rings"""

    def __init__(self, lib, b, n_cu, worst):
        self.b, self.n_cu, self.worst = b, n_cu, worst
        self.model = sc.context_model(lib)
        self.st = new_stream(lib, b)
        self._reset_oracle()

    def _reset_oracle(self):
        self.fed, self.only_ones = [], True
        self.step = vo.StepStream(self.b.net)

    def _check(self, n_new, what, step_ref=None):
        b = self.b
        p, z = self.st.read(want_logits=True)
        assert p.size == n_new, (what, p.size, n_new)
        if step_ref is not None:
            ref_z, ref_st = step_ref
        else:
            ref_z, ref_st = vo.whole_sequence(b.net, np.concatenate(self.fed, 0), rings=True)
            ref_z = ref_z[ref_z.size - n_new:]
        sc._compare(p, z, ref_z, what)
        if n_new:
            self.worst["logit"] = max(self.worst["logit"], float(np.abs(z - ref_z).max()))
        self.worst["state"] = max(self.worst["state"], sc.compare_state(self.st.get_state(), ref_st, b.net, what))

    def run(self, i):
        b, s = self.b, self.b.s
        st = b.case.script[i]
        what = "%s step %d %s" % (b.case.id, i, st[0])
        rng = sw._rng(b.case.id, 0, i)
        if st[0] == "reset":
            self.st.reset()
            self._reset_oracle()
        elif st[0] == "zero":
            before = self.st.get_state()
            n = self.st.run_host(sw.gen_frames(rng, s - 1))
            assert n == 0 and self.st.n_out == 0, what
            assert np.array_equal(before.view(np.uint8), self.st.get_state().view(np.uint8)), what + ": a call without outputs changed the state"
        elif st[0] == "tracks":
            tr = sc.Tracks(self.model, st[1], st[2], seed=int(rng.integers(1 << 30)))
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
            x = sw.gen_frames(rng, L, "u16" if i % 2 else "f32")
            n = self.st.run_host(x)
            assert n == L // s, what
            self.fed.append(x[:(L // s) * s])
            self.only_ones = False
            self._check(n, what)
        elif st[0] == "ones":
            for j in range(st[1]):
                x = sw.gen_frames(rng, s)
                assert self.st.run_host(x) == 1, what
                self.fed.append(x)
                ref = None
                if self.only_ones:   # the literal ring form, one step per chunk
                    ref = (np.array([self.step.step(x)]), self.step.state())
                self._check(1, "%s call %d" % (what, j), ref)
        else:
            raise ValueError(st)


def _chunking(lib, b):
    """``StreamingModel.predict_spectrogram`` over any split of the sequence gives bit for bit the probabilities and the final
    state of one call; a second run of the one call does too"""
    from microwakeword_amd import streaming

    def fresh():
        sm = object.__new__(streaming.StreamingModel)   # predict_spectrogram needs the native stream only
        sm.native = new_stream(lib, b)
        return sm

    n_out = len(b.seq) // b.s
    sm = fresh()
    p0 = sm.predict_spectrogram(b.seq)
    assert p0.size == n_out
    s0 = sm.native.get_state().view(np.uint8)
    sm.native.close()
    sm = fresh()
    assert np.array_equal(sm.predict_spectrogram(b.seq).view(np.uint32), p0.view(np.uint32)), b.case.id + ": reruns differ"
    assert np.array_equal(sm.native.get_state().view(np.uint8), s0), b.case.id + ": reruns differ (state)"
    sm.native.close()
    for si, pieces in enumerate(sw._splits(sw._rng(b.case.id, 77), n_out, b.s)):
        sm = fresh()
        ps = [sm.predict_spectrogram(b.seq[lo:hi]) for lo, hi in pieces]
        assert all(p.size == (hi - lo) // b.s for p, (lo, hi) in zip(ps, pieces))
        assert np.array_equal(np.concatenate(ps).view(np.uint32), p0.view(np.uint32)), "%s split %d %s: probabilities differ" % (
            b.case.id, si, pieces)
        assert np.array_equal(sm.native.get_state().view(np.uint8), s0), "%s split %d %s: final state differs" % (b.case.id, si, pieces)
        sm.native.close()


def _non_stream(lib, b, worst):
    """the non_stream twin against the non-streaming oracle model on every window; a second run bit for bit"""
    model = sc.context_model(lib)
    lens, pads = b.case.ns
    tr = sc.Tracks(model, lens, pads, seed=SEED)
    runs = []
    for _ in range(2):
        st = new_stream(lib, b, "non_stream")
        off = st.run(tr.win)
        runs.append(st.read(want_logits=True))
        st.close()
    p, z = runs[0]
    assert np.array_equal(p.view(np.uint32), runs[1][0].view(np.uint32)), b.case.id + ": non_stream reruns differ"
    for t, f in enumerate(tr.frames):
        ref = so.non_stream_windows(b.om, f.astype(np.float64), b.T, b.s)
        sc._compare(p[off[t]:off[t + 1]], z[off[t]:off[t + 1]], ref, "%s non_stream track %d" % (b.case.id, t))
        if ref.size:
            worst["logit"] = max(worst["logit"], float(np.abs(z[off[t]:off[t + 1]] - ref).max()))


def run_case(lib, c, n_cu=256):
    b = built(c.id)
    t0 = time.time()
    worst = {"logit": 0.0, "state": 0.0}
    if not c.desc["attention"]:
        ses = _Session(lib, b, n_cu, worst)
        for i in range(len(c.script)):
            ses.run(i)
        ses.st.close()
        _chunking(lib, b)
    _non_stream(lib, b, worst)
    return dict(id=c.id, seconds=time.time() - t0, logit_err=worst["logit"], state_err=worst["state"],
                logit_ratio=worst["logit"] / ec.FWD_TOL, state_ratio=worst["state"] / ec.FWD_TOL)


# ------------------------------------------------------------------------------------------ fixture and refusals
def check_reference_fixture(lib, golden_dir):
    """the ``mixednet_residual_heads`` case of tests/golden/ref_graph_golden.npz - residual 1,0,1,0, repeat 1,2,1,1,
    attention, max pool, T = 194; ``p_eval`` came out of the reference's own mixednet.py - through StreamingModel in
    non_stream mode: its weights in creation order, its three 194-frame inputs as three tracks"""
    import os
    from microwakeword_amd import mixednet, streaming
    name, T = "mixednet_residual_heads", 194
    flags = dict(mo.MIXEDNET_DEFAULTS, residual_connection="1,0,1,0", repeat_in_block="1,2,1,1", spatial_attention=1, pooled=1, max_pool=1)
    gold = np.load(os.path.join(golden_dir, "ref_graph_golden.npz"))
    n = sum(1 for k in gold.files if k.startswith(name + "/value/"))
    values = [gold["%s/value/%03d" % (name, i)] for i in range(n)]
    x, p_eval = gold[name + "/x"], gold[name + "/p_eval"]
    assert x.shape == (3, T, 40)
    model = mixednet.model(flags, (T, 40), 4, lib=lib, max_batch=4)
    model.set_weights(values)
    sm = streaming.StreamingModel(model, 1, "non_stream")
    assert sm.desc["residual"] == [1, 0, 1, 0] and sm.desc["attention"] == 1 and sm.desc["pool"] == "max" and sm.desc["t_final"] > 4
    model.engine.upload_store(1, np.concatenate([x.reshape(-1), np.zeros(40, np.float32)]).astype(np.float32))
    from microwakeword_amd import native
    win = np.array([(1, 0, T, 0, i * T * 40) for i in range(3)], native.WINDOW_DTYPE).reshape(-1)
    off = sm.native.run(win)
    assert list(off) == [0, 1, 2, 3]
    p = sm.read_probabilities()
    err = float(np.abs(p - p_eval).max())
    print("[mixednet_variant] fixture %s: |p - p_eval| max %.3e" % (name, err), flush=True)
    assert err <= ec.FWD_TOL, err
    return err


def check_abi_refusals(lib):
    """creation-time refusals of mww_stream_create_mixednet and the int8 entry points on such a stream"""
    import pytest
    from microwakeword_amd import native
    model = sc.context_model(lib)
    d = desc_of(6, 3, 1, [(1, (3,), 8)], 5, attention=1)
    ns = dict(d, mode="non_stream")
    native.Stream(model.engine, ns).close()
    with pytest.raises(native.NativeError, match="error -3.*non_stream mode only"):
        native.Stream(model.engine, dict(d, mode="stream"))                            # attention in stream mode
    with pytest.raises(native.NativeError, match="error -3.*t_final >= 4"):
        native.Stream(model.engine, dict(ns, t_final=3, frames=ns["frames"] - 2))     # T_f < 4 with attention
    with pytest.raises(native.NativeError, match="error -3.*does not match"):
        native.Stream(model.engine, dict(ns, t_final=6))                               # t_final does not match the window
    with pytest.raises(native.NativeError, match="error -3.*does not match"):
        native.Stream(model.engine, dict(desc_of(6, 3, 1, [(1, (3,), 8)], 5, pool="max"), mode="non_stream", t_final=1))
    with pytest.raises(native.NativeError, match="error -3.*pool"):
        native.Stream(model.engine, dict(ns, pool=7))                                  # a pool value outside 0..2
    with pytest.raises(native.NativeError, match="error -3.*ascending"):
        native.Stream(model.engine, dict(desc_of(6, 3, 1, [(1, (5, 3), 8)], 5, residual=[1])))
    # the six int8 entry points on a stream that uses one of the options: refused, naming the flags
    for dd in (desc_of(6, 3, 1, [(1, (3,), 8)], 3, residual=[1]), desc_of(6, 3, 1, [(1, (3,), 8)], 3, pool="average"), ns):
        st = native.Stream(model.engine, dd)
        st.set_weights(np.zeros(st.n_weights, np.float32))
        x, r = np.zeros((8, 40), np.float32), np.zeros((64, 2), np.float32)
        calibrate = lambda: st.nl.check(st.nl.lib.mww_stream_calibrate_host(st.h, native._fptr(x), 8, native._fptr(r)))   # noqa: E731
        calls = [st.num_tensors, calibrate, st.q8_sizes, lambda: st.read_q8(0), st.get_state_q8,
                 lambda: st.set_quantized(np.zeros(4, np.int8), np.zeros(4, np.int32), 1.0, np.zeros(256, np.uint8))]
        for call in calls:
            with pytest.raises(native.NativeError, match="error -3.*residual_connection, pooled or spatial_attention"):
                call()
        st.close()

