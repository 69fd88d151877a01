"""Host side of sharpness-aware steps and gradient clipping (microwakeword_amd/sharpness.py): the NumPy restatements against
scalar double arithmetic, the ``sharpness_aware`` / ``gradient_clipping`` mappings of the training configuration, and their
refusals - through the command line before ``train_dir`` exists, and for more than one rank.  No device."""
import math
import struct

import numpy as np
import pytest

import sharpness_checks as sc
from microwakeword_amd import sharpness


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def scalar_sumsq(g):
    """the definition, one CPython double operation at a time"""
    lanes = [0.0] * sharpness.LANES
    for i, v in enumerate(g):
        q = float(v) * float(v)
        lanes[i % sharpness.LANES] = lanes[i % sharpness.LANES] + q
    S = lanes[0]
    for s in lanes[1:]:
        S = S + s
    return S


def gradient(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 5, 1023, 1024, 1025, 22177])
def test_sumsq_is_the_lane_sums_folded_in_lane_order(n):
    g = gradient(n, seed=n)
    got = sharpness.sumsq(g)
    assert isinstance(got, float) and got == scalar_sumsq(g)
    assert abs(got - float(np.sum(g.astype(np.float64) ** 2))) <= 1e-12 * got   # (the order is part of the definition; the value is the sum)


def test_the_device_shapes_reach_the_lane_tails_and_the_scalar_tail():
    from microwakeword_amd.layout import InceptionLayout, MixedNetLayout
    import engine_checks as ec
    P = MixedNetLayout(ec.DEF, sc.T).n_params
    assert P == 22177 and P % 4 and P % sharpness.LANES and P > 4 * 256
    assert InceptionLayout(ec.INC, sc.T).n_params > sharpness.LANES


def test_perturbation_is_one_double_multiply_one_rounding_and_one_float_add():
    g, w = gradient(3000, 1), gradient(3000, 2)
    for rho in (0.05, 1e-3, 2.0):
        S = sharpness.sumsq(g)
        scale = rho / (math.sqrt(S) + 1e-12)
        assert sharpness.perturb_scale(S, rho) == scale
        want = np.array([np.float32(wi) + np.float32(_f32(scale * float(gi))) for wi, gi in zip(w, g)], np.float32)
        got = sharpness.perturb(w, g, rho)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # a zero gradient moves nothing (and divides by 1e-12, not by zero); a masked tap (g = 0) does not move
    assert sharpness.perturb(w, np.zeros_like(g), 0.05).tobytes() == (w + np.float32(0.0)).tobytes()
    g0 = g.copy()
    g0[::3] = 0.0
    assert np.array_equal(sharpness.perturb(w, g0, 0.05)[::3], w[::3])
    # nothing is screened
    bad = g.copy()
    bad[7] = np.nan
    assert np.isnan(sharpness.sumsq(bad)) and np.isnan(sharpness.perturb(w, bad, 0.05)).all()
    bad[7] = np.inf
    assert sharpness.sumsq(bad) == np.inf and sharpness.perturb_scale(np.inf, 0.05) == 0.0


def test_clipping_is_exact_at_or_below_the_threshold():
    g = gradient(5000, 3)
    S = sharpness.sumsq(g)
    norm = math.sqrt(S)
    for c in (norm, norm * 2, 1e30):
        assert sharpness.clip_factor(S, c) == 1.0
        assert sharpness.clip(g, c).tobytes() == g.tobytes()
    c = norm / 2
    k = c / norm
    assert sharpness.clip_factor(S, c) == k
    want = np.array([_f32(k * float(gi)) for gi in g], np.float32)
    got = sharpness.clip(g, c)
    assert got.tobytes() == want.tobytes()
    assert abs(math.sqrt(sharpness.sumsq(got)) - c) <= 1e-6 * c
    # a NaN norm compares false: k = 1, the gradient's bits stay; an infinite one scales finite entries to zero
    assert sharpness.clip_factor(float("nan"), 1.0) == 1.0 and sharpness.clip_factor(float("inf"), 1.0) == 0.0
    neg0 = np.array([-0.0, 1.0, np.nan], np.float32)
    assert sharpness.clip(neg0, 100.0).tobytes() == neg0.tobytes()


def test_training_config_mappings():
    assert (sharpness.SAM_KEY, sharpness.CLIP_KEY) == ("sharpness_aware", "gradient_clipping")
    assert sharpness.parse_config({}) == (None, None) and sharpness.parse_config({"sharpness_aware": None, "gradient_clipping": None}) == (None, None)
    assert sharpness.parse_sam_config({"sharpness_aware": dict(rho=0.05)}) == dict(rho=0.05, first_step=0)
    assert sharpness.parse_sam_config({"sharpness_aware": dict(rho=np.float32(0.5), first_step=np.int64(7))}) == dict(rho=0.5, first_step=7)
    assert sharpness.parse_clip_config({"gradient_clipping": dict(global_norm=1)}) == dict(global_norm=1.0)
    for bad, word in sc.BAD_SAM:
        with pytest.raises(ValueError, match="sharpness_aware.*" + word):
            sharpness.parse_config({"sharpness_aware": bad})
    for bad, word in sc.BAD_CLIP:
        with pytest.raises(ValueError, match="gradient_clipping.*" + word):
            sharpness.parse_config({"gradient_clipping": bad})


def test_more_than_one_rank_is_refused():
    both = {"sharpness_aware": dict(rho=0.05), "gradient_clipping": dict(global_norm=1.0)}
    assert sharpness.parse_config(both, 1) == (dict(rho=0.05, first_step=0), dict(global_norm=1.0))
    for key in both:
        with pytest.raises(ValueError, match=key + ".*single-device.*2 ranks"):
            sharpness.parse_config({key: both[key]}, 2)
    assert sharpness.parse_config({}, 2) == (None, None)


def test_the_loop_refuses_more_than_one_rank_before_the_first_step(monkeypatch):
    from microwakeword_amd import train as tr

    class Model:
        steps = 0

        def compile(self):
            pass

        def make_train_function(self):
            pass

        def train_on_batch(self, *a, **k):
            Model.steps += 1
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    for key, value in (("sharpness_aware", dict(rho=0.05)), ("gradient_clipping", dict(global_norm=1.0))):
        with pytest.raises(ValueError, match=key + ".*single-device"):
            tr.train(Model(), {key: value, "train_dir": "/nonexistent", "batch_size": 16}, object(), verbose=False)
    assert Model.steps == 0
    # ... and a model that is not this package's, with one rank
    monkeypatch.setattr(tr, "process_group", lambda: (0, 1))
    with pytest.raises(ValueError, match="single-device.*data_parallel"):   # the forced one-rank data-parallel path installs a hook too
        tr.train(Model(), {"gradient_clipping": dict(global_norm=1.0), "data_parallel": True, "train_dir": "/nonexistent", "batch_size": 16}, object(), verbose=False)
    with pytest.raises(ValueError, match="sharpness_aware needs this package's Model"):
        tr.train(Model(), {"sharpness_aware": dict(rho=0.05), "train_dir": "/nonexistent", "batch_size": 16}, object(), verbose=False)


def test_bad_mappings_are_refused_before_train_dir_exists(tmp_path):
    import yaml
    from microwakeword_amd import model_train_eval
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=16, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet", "--residual_connection", "0,0,0,0"]
    for key, cases in (("sharpness_aware", sc.BAD_SAM), ("gradient_clipping", sc.BAD_CLIP)):
        for bad, word in cases:
            with open(tmp_path / "training_parameters.yaml", "w") as out:
                yaml.safe_dump(dict(base, **{key: bad}), out)
            with pytest.raises(ValueError, match=key + ".*" + word):
                model_train_eval.main(argv)
            assert not train_dir.exists()
