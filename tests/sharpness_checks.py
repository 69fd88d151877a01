"""Checks of sharpness-aware train steps and global-norm gradient clipping (``mww_set_sharpness_aware`` / ``mww_set_grad_clip``
of the context core, csrc/kernels_sam.hip.h, ``microwakeword_amd/sharpness.py``), shared by tests/test_sharpness_emulated.py
(tests/hipemu) and tests/test_sharpness_gpu.py, the same shapes on both: B = 6, T = 194, two steps, the default MixedNet flags
(block kernels; P = 22 177, odd: the lane tails of the norm and the scalar tail of the elementwise kernels) and the default
Inception flags (graph kernels) - the sizes ``engine_checks.check_train_steps`` uses.

Every comparison but the float64-oracle one is byte for byte: the arithmetic between the backward pass and Adam is specified
operation for operation (``sharpness``), and everything else is "the same launches on the same inputs".
"""
import logging
import os

import numpy as np
import pytest
import torch

import engine_checks as ec
from microwakeword_amd import averaging, native, qat, sharpness
from microwakeword_amd.layout import InceptionLayout

B, T, STEPS, LR = 6, 194, 2, 1e-3
RHO = 0.05
KINDS = ("mixednet", "inception")
NO_APPLY, NO_METRICS = native.STEP_NO_APPLY, native.STEP_NO_METRICS


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(got, want, what):
    """tuples of arrays / scalars / bytes, element by element, naming the first that differs"""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(a, np.ndarray):
            if not same_bits(a, b):
                bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
                raise AssertionError("%s: item %d differs at %d of %d elements, first %d: %r vs %r" % (what, k, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))
        else:
            assert a == b, (what, k, a, b)


# ---------------------------------------------------------------------------------------------- engines, batches, steps
_START = {}


def oracle_of(kind):
    return ec.perturbed_oracle(T) if kind == "mixednet" else ec.perturbed_inception_oracle(T, ec.INC)


def start(lib, kind, prepare=None):
    """an engine of the family on engine_checks' perturbed weights, grids of two workgroups (three windows each)"""
    if kind not in _START:   # the weights once: every engine of a kind starts from the same bytes
        om = oracle_of(kind)
        lay = ec.MixedNetLayout(ec.DEF, T) if kind == "mixednet" else InceptionLayout(ec.INC, T)
        _START[kind] = lay.pack(om.get_weights())
    p, s = _START[kind]
    if kind == "mixednet":
        lay, eng = ec.make_engine(lib, T, B)
        grids = ("grid_fwd", "grid_bwd", "grid_head")
    else:
        lay = InceptionLayout(ec.INC, T)
        eng = native.Engine(lib=lib, **lay.engine_args(B))
        grids = ("grid_graph", "grid_head")
    eng.set_params(p)
    eng.set_bn_state(s)
    for g in grids:
        eng.set_option(g, 2)
    if prepare is not None:
        prepare(eng, lay)
    return lay, eng


def batches(kind, n=STEPS, seed=11):
    """(x, y, sample weights, pinned dropout mask or None) of n steps"""
    rng = np.random.default_rng(seed)
    out = []
    n_drop = None
    if kind == "inception":
        lay = InceptionLayout(ec.INC, T)
        n_drop = lay.t_last * lay.c_last
    for _ in range(n):
        x = ec.synth_x(rng, B, T)
        y = (rng.random(B) < 0.5).astype(np.float32)
        w = rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32)
        keep = (rng.random((B, n_drop)) >= ec.INC["dropout"]).astype(np.float32) if n_drop else None
        out.append((x, y, w, keep))
    return out


def give(eng, batch, lazy=False):
    """the batch becomes the engine's current one: a ready-made x, or (lazy) descriptors of windows in a resident store, which
    the first kernels gather through the mailbox slot"""
    x, y, w, keep = batch
    if lazy:
        eng.upload_store(0, x.reshape(-1))
        eng.set_targets(y, w)
        eng.assemble(np.array([(0, 0, T, 0, i * T * 40) for i in range(B)], native.WINDOW_DTYPE), None, 0, 0)
    else:
        eng.set_batch(x)
        eng.set_targets(y, w)
    if keep is not None:
        eng.set_dropout_mask(keep)


def step(eng, batch, flags=0, lazy=False):
    give(eng, batch, lazy)
    eng.train_step(B, LR, flags)


def snapshot(eng):
    m, v, n = eng.get_opt_state()
    return (eng.get_params(), m, v, np.int64(n), eng.get_bn_state(), bytes(eng.metrics_raw()), eng.get_grads())


def sam(rho=RHO, clip=0.0, graphs=0, weight_qat=False, ema=0.0):
    def prepare(eng, lay):
        if weight_qat:
            eng.set_weight_qat_map(*qat.channel_map(lay))
            eng.set_option("weight_qat", 1)
        if ema:
            eng.set_weight_ema(ema, 1)
        if rho:
            eng.set_sharpness_aware(rho)
        if clip:
            eng.set_grad_clip(clip)
        if graphs:
            eng.set_option("graphs", 1)
    return prepare


def write_grads(eng, g):
    """the engine's gradient buffer := g (what a data-parallel exchange does between a gradient-only step and apply_gradients)"""
    from microwakeword_amd import parallel
    eng.synchronize()
    ptr, n = eng.device_ptr(native.BUF_GRADS), eng.n_params
    src = torch.from_numpy(np.ascontiguousarray(g, np.float32))
    if eng.nl.host_emulated:
        parallel.host_floats(ptr, n).copy_(src)
    else:
        parallel.wrap_device_floats(ptr, n, torch.device("cuda", 0)).copy_(src)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 1. the twin, byte for byte
def twin_step(twin, batch, rho, clip=0.0, lazy=False):
    """the sharpness-aware step by hand on a plain engine: two gradient-only steps around the host's w', then Adam.
    -> (g(w), g(w') as Adam consumed it, S of g(w), S of g(w') before clipping)"""
    step(twin, batch, NO_APPLY, lazy)
    g1, w, bn_first = twin.get_grads(), twin.get_params(), twin.get_bn_state()
    S1 = sharpness.sumsq(g1)
    twin.set_params(sharpness.perturb(w, g1, rho, S1))
    twin.train_step(B, LR, NO_APPLY | NO_METRICS)   # the same batch (a descriptor-only one: its slot has moved on, x is written out)
    g2 = twin.get_grads()
    S2 = sharpness.sumsq(g2)
    twin.set_params(w)
    twin.set_bn_state(bn_first)   # (a gradient-only step updates the moving statistics; the second pass of the real step does not)
    if clip:
        g2 = sharpness.clip(g2, clip, S2)
        write_grads(twin, g2)
    twin.apply_gradients(LR, 1.0)
    return g1, g2, S1, S2


def check_twin(lib, kind, weight_qat=False, lazy=False, clip_factor=0.0):
    """check 1 (and, with weight_qat, check 5a; with clip_factor, SAM and clipping together at c = clip_factor x the norm)"""
    lay, eng = start(lib, kind, sam(weight_qat=weight_qat))
    _, twin = start(lib, kind, sam(rho=0.0, weight_qat=weight_qat))
    with pytest.raises(native.NativeError, match="error -4: .*grad_norms"):
        eng.get_grad_norms()
    moved = 0
    for k, b in enumerate(batches(kind)):
        clip = 0.0
        if clip_factor:   # the threshold from the measured norm of the second gradient, taken on a scratch copy of the twin
            _, probe = start(lib, kind, sam(rho=0.0, weight_qat=weight_qat))
            probe.set_params(twin.get_params())
            probe.set_bn_state(twin.get_bn_state())
            probe.set_opt_state(*twin.get_opt_state())
            clip = clip_factor * float(np.sqrt(twin_step(probe, b, RHO)[3]))
            probe.close()
            eng.set_grad_clip(clip)
        step(eng, b, lazy=lazy)
        g1, g2, S1, S2 = twin_step(twin, b, RHO, clip, lazy)
        what = "%s step %d" % (kind, k + 1)
        assert eng.get_grad_norms() == (S1, S2), (what, eng.get_grad_norms(), (S1, S2))
        assert S1 > 0 and np.isfinite(S1) and not same_bits(g1, g2)
        # gradient Adam consumed, parameters, Adam m / v / step, moving statistics of the first pass, metric counters of one pass
        got = snapshot(eng)
        assert_same(got[-1:] + got[:-1], (g2,) + snapshot(twin)[:-1], what)
        assert eng.get_opt_state()[2] == k + 1
        if clip_factor:
            assert (sharpness.clip_factor(S2, clip) < 1.0) == (clip_factor < 1.0)
        moved += int(np.count_nonzero(g1))
    assert moved
    eng.close()
    twin.close()
    return eng.n_params


def check_masked_taps_do_not_move(lib):
    """the default MixedNet has no structurally masked tap; the two-group MixConv of weight_qat_checks' small block model has:
    their gradient is 0, so neither the perturbation nor Adam moves them, whatever they hold"""
    import weight_ema_checks as we
    import weight_qat_checks as wq
    lay, eng = wq.new_engine(lib, "block")
    masked = lay.grad_mask() == 0
    assert masked.any()
    p, s = lay.pack(wq.random_weights(lay, 4))
    p[masked] = np.float32(-0.0)
    p[np.nonzero(masked)[0][::2]] = np.float32(3.5)
    eng.set_params(p)
    eng.set_bn_state(np.abs(s) + np.float32(0.5))
    eng.set_sharpness_aware(RHO)
    eng.set_grad_clip(1e-3)
    for b in we.batches(2):
        we.step(eng, b)
        assert not eng.get_grads()[masked].any()
        assert same_bits(eng.get_params()[masked], p[masked]) and not same_bits(eng.get_params(), p)
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. the float64 oracle at w'
def check_oracle_at_the_perturbed_point(lib, kind):
    """The gradient a sharpness-aware step hands to Adam against the float64 oracle's gradient at the device's own fp32 w' (the
    restatement's w', which check 1 holds the device to bit for bit), with the fp32 bounds - and the imposed ReLU decisions - of
    ``engine_checks._check_train_steps`` / ``check_inception_train_steps``.  Those comparisons are inline in functions that also
    compare a plain step's parameters, moving statistics and metric counters, which are another step's here; the gradient part
    is restated below with their numbers, none of its own."""
    lay, eng = start(lib, kind, sam())
    _, twin = start(lib, kind)
    om = oracle_of(kind)
    inception = kind == "inception"
    l2s = []
    for s, b in enumerate(batches(kind)):
        x, y, w, keep = b
        w_master, state = eng.get_params(), eng.get_bn_state()   # the twin takes the first gradient from the engine's own weights
        twin.set_params(w_master)
        twin.set_bn_state(state)
        step(twin, b, NO_APPLY)
        g_first = twin.get_grads()
        w_prime = sharpness.perturb(w_master, g_first, RHO)
        step(eng, b)
        om.set_weights(lay.unpack(w_prime, state))
        kw = dict(dropout_mask=keep) if inception else {}
        pr, z, loss = eng.read_outputs(B)   # the last forward's: the second pass
        taps, masks, flips = {}, {}, 0
        om.logits(x, True, taps=taps, **kw)
        if inception:
            for k, (members, op) in enumerate(zip(lay.op_members, lay.ops)):
                n_el = B * op["tout"] * op["filters"]
                pk = eng.debug_read("p%d" % (k + 1), B, n_el).reshape(B, op["tout"], op["filters"]).astype(np.float64)
                bn = eng.debug_read("bn%d" % (k + 1), B, 9 * op["filters"]).reshape(9, op["filters"]).astype(np.float64)
                m_all = (pk * bn[0] + bn[1]) > 0
                for name, c0, cn in members:
                    m = m_all[:, :, c0:c0 + cn]
                    ref = taps[name + ".bn_out"].detach().numpy()
                    diff = m != (ref > 0)
                    flips += int(diff.sum())
                    assert np.abs(ref[diff]).max(initial=0.0) <= 2e-5 * max(1.0, np.abs(ref).max()), (name, np.abs(ref[diff]).max())
                    masks[name] = np.ascontiguousarray(m.transpose(0, 2, 1))
            n_units = sum(B * op["tout"] * op["filters"] for op in lay.ops)
        else:
            ref0 = taps["conv1.pre"].detach().numpy()
            a0 = eng.debug_read("a0", B, ref0.size).reshape(ref0.shape)
            d0 = (a0 > 0) != (ref0 > 0)
            flips += int(d0.sum())
            assert np.abs(ref0[d0]).max(initial=0.0) <= 2e-5 * max(1.0, np.abs(ref0).max()), np.abs(ref0[d0]).max()
            masks["conv1"] = np.ascontiguousarray((a0 > 0).transpose(0, 2, 1))
            for k, blk in enumerate(lay.blocks):
                pk = eng.debug_read("p%d" % (k + 1), B, B * blk.tout * blk.cout).reshape(B, blk.tout, blk.cout).astype(np.float64)
                bn = eng.debug_read("bn%d" % (k + 1), B, 9 * blk.cout).reshape(9, blk.cout).astype(np.float64)
                m = (pk * bn[0] + bn[1]) > 0
                ref = taps["b%d.r0.bn_out" % k].detach().numpy()
                diff = m != (ref > 0)
                flips += int(diff.sum())
                assert np.abs(ref[diff]).max(initial=0.0) <= 2e-5 * max(1.0, np.abs(ref).max()), (k, np.abs(ref[diff]).max())
                masks["b%d.r0" % k] = np.ascontiguousarray(m.transpose(0, 2, 1))
            n_units = sum(B * blk.tout * blk.cout for blk in lay.blocks)
        assert flips <= max(8, 2e-5 * n_units), flips
        lo, po, grads, _ = om.loss_and_grads(x, y, w, relu_masks=masks, **kw)
        g = eng.get_grads()
        if inception:
            gref = lay.pack([grads[n].numpy().astype(np.float32) if vk == "param" else np.zeros(shape, np.float32) for n, shape, vk in lay.keras_vars])[0]
        else:
            gref = ec.oracle_grads_native_order(lay, om, grads)
        print("%s step %d: loss %.7f vs %.7f, max |dp| %.2e, max |dg| / max |g| %.2e" % (kind, s + 1, loss, lo, np.abs(pr - po).max(),
                                                                                    np.abs(g - gref).max() / max(1e-6, np.abs(gref).max())))
        assert abs(loss - lo) <= 1e-5 * max(1.0, abs(lo)), (loss, lo)
        assert np.abs(pr - po).max() <= ec.FWD_TOL
        scale = max(1e-6, float(np.abs(gref).max()))
        off = 0
        for name, n in lay.segments():
            a, r = g[off:off + n], gref[off:off + n]
            off += n
            if not inception and name.endswith("dw.bias"):
                assert np.abs(a - r).max() <= 2e-3 * scale, (s, name, np.abs(a - r).max(), scale)
                continue
            seg_scale = max(float(np.abs(r).max()), 1e-3 * scale)
            l2 = float(np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-3 * scale * np.sqrt(n)))
            loose = name == "dense.bias" or name.endswith((".bn.gamma", ".bn.beta"))
            assert l2 <= (1e-3 if loose else 1e-4), (s, name, l2)
            assert np.abs(a - r).max() <= 1e-3 * seg_scale, (s, name, np.abs(a - r).max(), seg_scale)
            l2s.append(l2)
        # the comparison has teeth: the gradient at w itself is far outside the bound on a tensor's relative L2 error
        assert np.linalg.norm(g_first - gref) / np.linalg.norm(gref) > 1e-2
    assert np.median(l2s) <= 2e-5, (np.median(l2s), max(l2s))
    eng.close()
    twin.close()
    return max(l2s)


# ---------------------------------------------------------------------------------------------- 3. observing only
def check_observing_only(lib, kind, graphs=0):
    def toggled(eng, lay):
        if graphs:
            eng.set_option("graphs", 1)
        eng.set_sharpness_aware(RHO)
        eng.set_grad_clip(1.0)
        eng.set_sharpness_aware(0.0)
        eng.set_grad_clip(0.0)

    def plain(eng, lay):
        if graphs:
            eng.set_option("graphs", 1)

    def removed_midway(eng, lay):   # one sharpened, clipped step on another batch, then everything put back
        plain(eng, lay)
        eng.set_sharpness_aware(RHO)
        eng.set_grad_clip(1e-3)
        p, s, opt = eng.get_params(), eng.get_bn_state(), eng.get_opt_state()
        step(eng, batches(kind, 1, seed=3)[0])
        eng.set_sharpness_aware(0.0)
        eng.set_grad_clip(0.0)
        eng.set_params(p)
        eng.set_bn_state(s)
        eng.set_opt_state(*opt)
        eng.metrics_reset()
    runs = []
    for prepare in (plain, toggled, removed_midway):
        lay, eng = start(lib, kind, prepare)
        outs = []
        for b in batches(kind):
            step(eng, b)
            outs.append(eng.read_outputs(B)[0])
        runs.append(snapshot(eng) + tuple(outs))
        with pytest.raises(native.NativeError, match="error -4: .*grad_norms"):
            eng.get_grad_norms()   # (removing both forgets the norms)
        eng.close()
    assert all(np.all(np.isfinite(a)) for a in runs[0] if isinstance(a, np.ndarray))
    assert_same(runs[1], runs[0], kind + ": installed and removed")
    assert_same(runs[2], runs[0], kind + ": removed after a step")   # (dropout masks are pinned: no generator counter to put back)


# ---------------------------------------------------------------------------------------------- 4. clipping
def check_clipping(lib, kind):
    bs = batches(kind)
    _, probe = start(lib, kind)
    step(probe, bs[0], NO_APPLY)
    g = probe.get_grads()
    S = sharpness.sumsq(g)
    norm = float(np.sqrt(S))
    # active: half the measured norm
    c = norm / 2
    lay, eng = start(lib, kind, sam(rho=0.0, clip=c))
    step(eng, bs[0])
    want = sharpness.clip(g, c, S)
    assert sharpness.clip_factor(S, c) < 1.0 and not same_bits(want, g)
    assert_same((eng.get_grads(),), (want,), kind + ": clipped gradient")
    assert eng.get_grad_norms() == (S, S)
    write_grads(probe, want)
    probe.apply_gradients(LR, 1.0)
    assert_same(snapshot(eng)[:-1], snapshot(probe)[:-1], kind + ": clipped step against apply_gradients on the restated gradient")
    # ... and in front of Adam in apply_gradients: the two-call form of the same step
    _, two = start(lib, kind, sam(rho=0.0, clip=c))
    step(two, bs[0], NO_APPLY)
    assert same_bits(two.get_grads(), g)   # a gradient-only step is never clipped
    two.apply_gradients(LR, 1.0)
    assert_same(snapshot(two), snapshot(eng), kind + ": clipping in apply_gradients")
    assert two.get_grad_norms() == (S, S)
    # inactive: twice the largest norm the plain run measures - the bytes of the plain fused step, gradient included
    _, plain = start(lib, kind)
    want = []
    for b in bs:
        step(plain, b)
        want.append(snapshot(plain))
    norms = [float(np.sqrt(sharpness.sumsq(w[-1]))) for w in want]
    _, off = start(lib, kind, sam(rho=0.0, clip=2 * max(norms)))
    for k, b in enumerate(bs):
        step(off, b)
        assert_same(snapshot(off), want[k], "%s: clipping at or below the threshold, step %d" % (kind, k + 1))
        assert off.get_grad_norms() == (sharpness.sumsq(want[k][-1]),) * 2
    assert sharpness.clip_factor(S, 2 * norm) == 1.0 and sharpness.clip_factor(S, norm) == 1.0
    for e in (probe, eng, two, off, plain):
        e.close()


# ---------------------------------------------------------------------------------------------- 5. interplay
def check_with_weight_average(lib, kind):
    """one update of the average per step, behind the restore: averaging.ema_update of the final parameters"""
    decay = 0.9
    lay, eng = start(lib, kind, sam(ema=decay, clip=1e-3))
    masters = []
    for k, b in enumerate(batches(kind)):
        step(eng, b)
        masters.append(eng.get_params())
        ema, n = eng.get_ema_state()
        want, updates = averaging.ema_fold(masters, decay)
        assert n == updates == k + 1
        assert_same((ema,), (want,), "%s: average after step %d" % (kind, k + 1))
    assert not same_bits(masters[0], masters[1])
    eng.close()


def check_graphs_option(lib, kind):
    """under "graphs" 1 a step with either feature gives the bytes of the eager step; installing drops the captured steps"""
    bs = batches(kind, 3)
    for rho, clip in ((RHO, 0.0), (0.0, 1e-3), (RHO, 1e-3)):
        finals = []
        for graphs in (0, 1):
            lay, eng = start(lib, kind, lambda e, l: e.set_option("graphs", graphs))
            step(eng, bs[0])       # a plain step: captured under "graphs"
            sam(rho, clip)(eng, lay)
            for b in bs[1:]:
                step(eng, b)
            finals.append(snapshot(eng) + eng.get_grad_norms())
            eng.close()
        assert_same(finals[1], finals[0], "%s rho %g clip %g" % (kind, rho, clip))


def check_non_finite(lib, kind):
    """a NaN planted through the batch - in the spectrogram, in a sample weight - leaves NaN parameters where a plain step
    leaves NaN parameters, and the call returns MWW_OK.  (Where a ReLU swallows the spectrogram's NaN, the plain step stays finite and
    that plant shows nothing; the sample weight's reaches every gradient.)"""
    reached = 0
    for plant in ("x", "weight"):
        x, y, w, keep = batches(kind, 1)[0]
        x, w = x.copy(), w.copy()
        if plant == "x":
            x[0, 5, 7] = np.nan
        else:
            w[0] = np.nan
        got = []
        for prepare in (None, sam(), sam(clip=1.0)):
            lay, eng = start(lib, kind, prepare)
            step(eng, (x, y, w, keep))   # (a failing call raises)
            got.append(eng.get_params())
            if prepare is not None and np.isnan(got[0]).any():
                assert np.isnan(eng.get_grad_norms()[0])
            eng.close()
        # w' is NaN everywhere, so the second gradient is NaN wherever NaN gets past the ReLUs of an all-NaN forward - the
        # classifier at least, not necessarily every parameter the plain step loses: the run looks diverged, as the plain one does
        if np.isnan(got[0]).any():
            reached += 1
            assert np.isnan(got[1]).any() and np.isnan(got[2]).any(), (kind, plant)
    assert reached, kind


# ---------------------------------------------------------------------------------------------- 6. refusals
def check_refusals(lib, kind):
    bs = batches(kind)
    lay, fresh = start(lib, kind)
    step(fresh, bs[0])
    want = snapshot(fresh)
    fresh.close()

    def no(call, code, word):
        with pytest.raises(native.NativeError, match="error %d: .*%s" % (code, word)):
            call()
    lay, eng = start(lib, kind)
    for v in (-0.1, -1e-300, float("nan"), float("inf"), -float("inf")):
        no(lambda: eng.set_sharpness_aware(v), -1, "rho")
        no(lambda: eng.set_grad_clip(v), -1, "global_norm")
    no(lambda: eng.get_grad_norms(), -4, "grad_norms")
    # install next to a hook
    calls = []
    eng.set_allreduce_hook(lambda ptr, n, flags: calls.append(n), world_size=1, sync_bn=False, reduce_grads=True)
    no(lambda: eng.set_sharpness_aware(RHO), -3, "single-device")
    no(lambda: eng.set_grad_clip(1.0), -3, "single-device")
    eng.set_sharpness_aware(0.0)   # removing nothing is fine
    eng.set_allreduce_hook(None)
    step(eng, bs[0])
    assert_same(snapshot(eng), want, kind + ": after the refusals")   # the context is as it was: the step of a fresh context
    assert not calls
    eng.close()
    # a hook next to an installed feature; the refusals leave the feature on and the context usable
    lay, eng = start(lib, kind, sam(clip=1e-3))
    _, ref = start(lib, kind, sam(clip=1e-3))
    no(lambda: eng.set_allreduce_hook(lambda ptr, n, flags: calls.append(n), world_size=1, sync_bn=False, reduce_grads=True), -3, "single-device")
    no(lambda: eng.allreduce_init(0, 1, np.zeros(native.UNIQUE_ID_BYTES, np.uint8)), -3, "single-device")
    for v in (-1.0, float("nan")):
        no(lambda: eng.set_sharpness_aware(v), -1, "rho")
        no(lambda: eng.set_grad_clip(v), -1, "global_norm")
    for b in bs:
        step(eng, b)
        step(ref, b)
    assert_same(snapshot(eng) + eng.get_grad_norms(), snapshot(ref) + ref.get_grad_norms(), kind + ": refused hooks")
    assert not calls
    eng.get_grad_norms()
    eng.nl.check(eng.nl.lib.mww_get_grad_norms(eng.h, None, None))   # either pointer may be NULL
    eng.close()
    ref.close()


# ---------------------------------------------------------------------------------------------- 7. the loop
FIRST_STEP = 5


def loop_config(tmp_path, name, sam_map=None, clip_map=None, **over):
    import stream_mine_checks as smc
    cfg = dict(smc.loop_config(tmp_path, name), prefetch_batches=0, **over)
    if sam_map is not None:
        cfg["sharpness_aware"] = sam_map
    if clip_map is not None:
        cfg["gradient_clipping"] = clip_map
    return cfg


def arrays_of(path):
    with np.load(path + ".npz") as z:
        return [z[k].tobytes() for k in sorted(z.files)]


def summary_of(model):
    lines = []
    model.summary(print_fn=lines.append)
    return lines


def loop_files(cfg):
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    names = ["last_weights.weights.h5", "best_weights.weights.h5", os.path.join("restore", "ckpt.weights")]
    names += [os.path.relpath(svc.weights_at(cfg, k), cfg["train_dir"]) for k in svc.BOUNDARIES[:-1]]
    assert svc.BOUNDARIES[-1] == smc.STEPS
    return {name: arrays_of(os.path.join(cfg["train_dir"], name)) for name in names}


def check_loop(lib, tmp_path, caplog):
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    cfg = loop_config(tmp_path, "sharp", dict(rho=RHO, first_step=FIRST_STEP), dict(global_norm=0.05))
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        model, _ = smc.run_loop(lib, cfg)
    said = [r.getMessage() for r in caplog.records if "sharpness-aware" in r.getMessage()]
    assert len(said) == 1 and said[0].startswith("Step #%d: sharpness-aware steps on (rho %g" % (FIRST_STEP, RHO)), said
    assert any("gradient clipping on (global norm 0.05)" in r.getMessage() for r in caplog.records)
    log = svc.log_of(cfg, "train")
    assert [(e["step"], e["sharpness_aware"]) for e in log] == [(4, 0), (8, 1), (12, 1)]
    assert all(np.isfinite(e["grad_norm"]) and e["grad_norm"] > 0 for e in log)
    assert log[-1]["grad_norm"] == model.gradient_norms()[0] == float(np.sqrt(model.engine.get_grad_norms()[0]))
    lines = summary_of(model)
    assert any("sharpness-aware" in line and "0.05" in line for line in lines) and any("Gradient clipping" in line for line in lines)
    assert model.engine.get_opt_state()[2] == smc.STEPS
    plain = loop_config(tmp_path, "plain")
    smc.run_loop(lib, plain)
    assert loop_files(cfg)["last_weights.weights.h5"] != loop_files(plain)["last_weights.weights.h5"]
    # restored from the checkpoint of a run stopped behind step 8: on / off follows from the restored step, no second log line
    # about a first step in the past being reached "now" at a wrong step number
    cut = loop_config(tmp_path, "cut", dict(rho=RHO, first_step=FIRST_STEP), dict(global_norm=0.05), training_steps=[6, 2])
    smc.run_loop(lib, cut)
    rest = dict(cut, training_steps=[1], learning_rates=[cfg["learning_rates"][1]])
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        restored, _ = smc.run_loop(lib, rest)
    said = [r.getMessage() for r in caplog.records if "sharpness-aware" in r.getMessage()]
    assert len(said) == 1 and said[0].startswith("Step #9: sharpness-aware steps on"), said
    assert restored.engine.get_opt_state()[2] == 9 and restored.sharpness_aware == RHO


def check_loop_without_the_keys(lib, tmp_path):
    """no keys: the files of a run in which the options never existed - a second run whose first_step lies beyond its last step
    never installs the sharpness-aware step, a third clips at a threshold no gradient reaches; the train scalars of the first
    carry neither field"""
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    cfg = loop_config(tmp_path, "plain")
    model, _ = smc.run_loop(lib, cfg)
    assert not getattr(model, "sharpness_aware", None) and not getattr(model, "gradient_clipping", None)
    assert all("sharpness_aware" not in e and "grad_norm" not in e for e in svc.log_of(cfg, "train"))
    assert not any("sharpness-aware" in line or "Gradient clipping" in line for line in summary_of(model))
    with pytest.raises(native.NativeError, match="error -4: .*grad_norms"):
        model.engine.get_grad_norms()
    late = loop_config(tmp_path, "late", dict(rho=RHO, first_step=smc.STEPS + 1))
    model_l, _ = smc.run_loop(lib, late)
    assert [e["sharpness_aware"] for e in svc.log_of(late, "train")] == [0, 0, 0] and all("grad_norm" not in e for e in svc.log_of(late, "train"))
    assert not getattr(model_l, "sharpness_aware", None)
    high = loop_config(tmp_path, "high", None, dict(global_norm=1e30))
    model_h, _ = smc.run_loop(lib, high)
    assert model_h.gradient_clipping == 1e30 and all(e["grad_norm"] > 0 for e in svc.log_of(high, "train"))
    want = loop_files(cfg)
    for other in (late, high):
        got = loop_files(other)
        for name in want:
            assert got[name] == want[name], (other["train_dir"], name)
        with np.load(os.path.join(cfg["train_dir"], "restore", "ckpt.opt.npz")) as a, np.load(os.path.join(other["train_dir"], "restore", "ckpt.opt.npz")) as b:
            assert sorted(a.files) == sorted(b.files) == ["lr", "m", "step", "v"] and all(a[k].tobytes() == b[k].tobytes() for k in a.files)


BAD_SAM = ((dict(first_step=3), "rho"), (dict(rho=0.0), "rho"), (dict(rho=-0.1), "rho"), (dict(rho="0.05"), "rho"), (dict(rho=True), "rho"),
           (dict(rho=float("nan")), "rho"), (dict(rho=float("inf")), "rho"), (dict(rho=0.05, first_step=-1), "first_step"),
           (dict(rho=0.05, first_step=2.5), "first_step"), (dict(rho=0.05, first_step=True), "first_step"), (dict(rho=0.05, adaptive=True), "adaptive"),
           ([0.05, 3], "mapping"), (0.05, "mapping"))
BAD_CLIP = ((dict(), "global_norm"), (dict(global_norm=0.0), "global_norm"), (dict(global_norm=-1.0), "global_norm"),
            (dict(global_norm="1"), "global_norm"), (dict(global_norm=True), "global_norm"), (dict(global_norm=float("nan")), "global_norm"),
            (dict(global_norm=float("inf")), "global_norm"), (dict(global_norm=1.0, per_tensor=True), "per_tensor"), (1.0, "mapping"))
