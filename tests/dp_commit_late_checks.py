"""Shared by test_dp_commit_late_gpu.py and test_dp_commit_late_emulated.py: the engine option "dp_commit_late" is a schedule,
not arithmetic - the backward kernels commit the dp rows of a tile behind the depthwise recompute (1) or with the input rows in
front of it (0) - so everything a train step produces must agree bit for bit between the two orders."""
import numpy as np

import engine_checks as ec

K17_19 = dict(ec.DEF, mixconv_kernel_sizes="[5],[17],[19],[21]")   # square 48-wide blocks: two tap groups (17, 19) and the relane path (>= 15)

_weights = {}


def _packed_weights(flags, T):
    """the perturbed oracle's weights in engine order, built once per (topology, length) and never modified"""
    key = (tuple(sorted((k, str(v)) for k, v in flags.items())), T)
    if key not in _weights:
        lay = ec.MixedNetLayout(flags, T)
        p, s = lay.pack(ec.perturbed_oracle(T, flags=flags).get_weights())
        p.setflags(write=False)
        s.setflags(write=False)
        _weights[key] = (p, s)
    return _weights[key]


def train_arrays(lib, flags, B, T, late, grid=2, steps=2, options=None):
    """`steps` train steps from the same weights on the same batches; every array a step leaves behind"""
    p, s = _packed_weights({k: v for k, v in flags.items() if k not in ("bwd_wide", "conv1_x6", "bwd_first_wide", "conv1_x6_fwd")}, T)
    lay, eng = ec.make_engine(lib, T, B, None, flags=flags)
    try:
        eng.set_params(np.array(p))
        eng.set_bn_state(np.array(s))
        for k in ("grid_fwd", "grid_bwd", "grid_head"):
            eng.set_option(k, grid)
        for k, v in (options or {}).items():
            eng.set_option(k, v)
        eng.set_option("dp_commit_late", late)
        rng = np.random.default_rng(11)
        out = {}
        for step in range(steps):
            x = ec.synth_x(rng, B, T)
            y = (rng.random(B) < 0.5).astype(np.float32)
            w = rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32)
            eng.set_batch(x)
            eng.set_targets(y, w)
            eng.train_step(B, 1e-3)
            pr, z, loss = eng.read_outputs(B)
            out["prob%d" % step], out["logit%d" % step], out["loss%d" % step] = pr.copy(), z.copy(), np.float64(loss)
            out["grad%d" % step] = eng.get_grads().copy()
            out["param%d" % step] = eng.get_params().copy()
            out["bn%d" % step] = eng.get_bn_state().copy()
        return out
    finally:
        eng.close()


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max()))
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in a.values()), what
    assert any(np.any(a[k] != 0) for k in a if k.startswith("grad")), what


def check_late_equals_early(lib, flags, B, T, grid=2, steps=2, options=None):
    early = train_arrays(lib, flags, B, T, 0, grid, steps, options)
    late = train_arrays(lib, flags, B, T, 1, grid, steps, options)
    assert_same_bits(early, late, (T, options))
    return late
