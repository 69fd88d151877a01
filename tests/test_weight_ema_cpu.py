"""Host side of weight averaging (microwakeword_amd/averaging.py): the NumPy restatement of the update against scalar double
arithmetic, the ``weight_averaging`` mapping of the training configuration, and its refusal through the command line before
``train_dir`` exists.  No device."""
import struct

import numpy as np
import pytest

import weight_ema_checks as we
import weight_qat_checks as wq
from microwakeword_amd import averaging


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def test_first_update_is_a_bit_copy():
    w = np.array([1.5, -0.0, np.nan, np.inf, 1e-40, -3.25], np.float32)
    for ema in (None, np.zeros(6, np.float32)):
        got = averaging.ema_update(ema, w, 0.999, 0)
        assert got.dtype == np.float32 and got.tobytes() == w.tobytes() and got is not w


def test_update_is_three_double_operations_and_one_rounding():
    rng = np.random.default_rng(0)
    e = (rng.normal(0, 1, 4096) * 10.0 ** rng.integers(-6, 3, 4096)).astype(np.float32)
    w = (e + rng.normal(0, 1, 4096).astype(np.float32) * np.abs(e) * np.float32(1e-2)).astype(np.float32)
    for decay in (0.9, 0.999, 0.5, 1e-3):
        om = 1.0 - decay
        got = averaging.ema_update(e, w, decay, 5)
        # CPython floats are doubles and `a + b * c` is two roundings there: the specified arithmetic, element by element
        want = np.array([_f32(float(ei) + om * (float(wi) - float(ei))) for ei, wi in zip(e, w)], np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # not the float32 form of the same expression (the update would lose the small differences a long average is made of)
    f32 = e + np.float32(1.0 - 0.999) * (w - e)
    assert averaging.ema_update(e, w, 0.999, 5).tobytes() != f32.tobytes()
    # a constant master is a fixed point, bit for bit (the masked MixConv taps of a MixedNet stay what the master holds)
    assert averaging.ema_update(e, e, 0.9, 3).tobytes() == e.tobytes()


def test_non_finite_values_propagate():
    e = np.array([1.0, 1.0, 1.0, np.inf, np.nan], np.float32)
    w = np.array([np.inf, -np.inf, np.nan, 1.0, 1.0], np.float32)
    got = averaging.ema_update(e, w, 0.9, 1)
    assert got[0] == np.inf and got[1] == -np.inf and np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(got[4])
    big = averaging.ema_update(np.array([3e38], np.float32), np.array([-3e38], np.float32), 0.5, 1)   # finite in double
    assert big[0] == 0.0


def test_fold_counts_the_steps_that_are_multiples_of_the_period():
    ws = [np.full(3, k, np.float32) for k in range(1, 7)]
    ema, n = averaging.ema_fold(ws, 0.5, every_steps=2)
    assert n == 3 and ema.tolist() == [4.5] * 3   # 2 -> (2 + 4) / 2 = 3 -> (3 + 6) / 2
    ema, n = averaging.ema_fold(ws[:2], 0.5, every_steps=3)
    assert n == 0 and ema is None
    a, n = averaging.ema_fold(ws[:3], 0.5)
    b, m = averaging.ema_fold(ws[3:], 0.5, first_opt_step=4, ema=a, updates=n)
    c, k = averaging.ema_fold(ws, 0.5)
    assert m == k == 6 and b.tobytes() == c.tobytes()


def test_the_three_models_reach_the_vector_loop_and_the_scalar_tail():
    """the shapes the device checks run: parameter counts beyond one workgroup (256 threads x 4 floats), at least one that is
    no multiple of four (scalar tail) and none that is a multiple of the workgroup's reach"""
    counts = {kind: wq.layout_of(kind).n_params for kind in we.KINDS}
    assert all(n > 1024 and n % 1024 for n in counts.values()), counts
    assert any(n % 4 for n in counts.values()), counts


def test_training_config_mapping():
    key = averaging.CONFIG_KEY
    assert key == "weight_averaging"
    assert averaging.parse_config({}) is None and averaging.parse_config({key: None}) is None
    assert averaging.parse_config({key: dict(decay=0.999, first_step=100)}) == dict(decay=0.999, first_step=100, every_steps=1)
    assert averaging.parse_config({key: dict(decay=np.float32(0.5), first_step=np.int64(0), every_steps=10)}) == dict(decay=0.5, first_step=0, every_steps=10)
    for bad, word in we.BAD_MAPPINGS:
        with pytest.raises(ValueError, match="weight_averaging.*" + word):
            averaging.parse_config({key: bad})


def test_bad_mappings_are_refused_before_train_dir_exists(tmp_path):
    import yaml
    from microwakeword_amd import model_train_eval
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=16, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet", "--residual_connection", "0,0,0,0"]
    for bad, word in we.BAD_MAPPINGS:
        with open(tmp_path / "training_parameters.yaml", "w") as out:
            yaml.safe_dump(dict(base, weight_averaging=bad), out)
        with pytest.raises(ValueError, match="weight_averaging.*" + word):
            model_train_eval.main(argv)
        assert not train_dir.exists()
