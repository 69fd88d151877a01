"""Host side of weight-only quantization-aware training (microwakeword_amd/qat.py): the channel map of every layout, the NumPy
restatement of the shadow, the ``weight_quantization_aware`` mapping of the training configuration.  No device."""
import numpy as np
import pytest

import stream_sweep as ss
import streaming_checks as sc
import weight_qat_checks as wq
from microwakeword_amd import qat, quantize
from microwakeword_amd.layout import GraphMixedNetLayout


def _layouts():
    out = [(kind, wq.layout_of(kind)) for kind in wq.KINDS]
    out += [(c.id, GraphMixedNetLayout(sc.flags_of(c.desc), int(c.desc["frames"]))) for c in ss.cases()]   # the topology axes of the stream sweep
    return out


LAYOUTS = _layouts()


@pytest.mark.parametrize("name,lay", LAYOUTS, ids=[n for n, _ in LAYOUTS])
def test_channel_map_covers_every_kernel_element_once_and_nothing_else(name, lay):
    start, elem = qat.channel_map(lay)
    assert start.dtype == np.int32 and elem.dtype == np.int32 and start[0] == 0 and start[-1] == elem.size
    assert np.all(np.diff(start) > 0) and elem.min() >= 0 and elem.max() < lay.n_params
    assert np.unique(elem).size == elem.size   # no element in two channels
    # independently: kernels packed as ones, everything else as zeros - the channel elements are exactly the ones (biases, BN
    # variables and the masked MixConv taps, which no Keras element reaches, are outside)
    axes = [qat.kernel_axis(n, s) if kind == "param" else None for n, s, kind in lay.keras_vars]
    ones = lay.pack([np.full(s, 0.0 if a is None else 1.0, np.float32) for (_, s, _), a in zip(lay.keras_vars, axes)])[0]
    inside = np.zeros(lay.n_params, bool)
    inside[elem] = True
    assert np.array_equal(inside, ones == 1.0)
    assert elem.size == sum(int(np.prod(s)) for (_, s, _), a in zip(lay.keras_vars, axes) if a is not None)
    assert all(a is not None for (n, s, _), a in zip(lay.keras_vars, axes) if len(s) == 4 or n == "dense.kernel")
    assert not any(inside[lay.grad_mask() == 0])
    # every channel holds the elements of one output channel of one tensor: member count = size / channels
    tags, sizes, c = [], [], 0
    for (n, s, _), a in zip(lay.keras_vars, axes):
        t = np.zeros(s, np.float32)
        if a is not None:
            shape = [1] * len(s)
            shape[a] = -1
            t = t + np.arange(c + 1, c + 1 + s[a], dtype=np.float32).reshape(shape)
            sizes += [int(np.prod(s)) // s[a]] * s[a]
            c += s[a]
        tags.append(t)
    packed = lay.pack(tags)[0]
    assert start.size - 1 == c
    for ch in range(c):
        members = elem[start[ch]:start[ch + 1]]
        assert members.size == sizes[ch] and np.all(packed[members] == ch + 1), (name, ch)


def test_kernel_axes_are_the_quantizers():
    assert qat.kernel_axis("conv1.kernel", (3, 1, 40, 32)) == 3 and qat.kernel_axis("b0.r1.dw0.kernel", (5, 1, 24, 1)) == 2
    assert qat.kernel_axis("b1.dw1.kernel", (11, 1, 16, 1)) == 2 and qat.kernel_axis("dense.kernel", (96, 1)) == 1
    assert qat.kernel_axis("attention.kernel", (4, 1, 2, 1)) == 3 and qat.kernel_axis("i0.red.kernel", (1, 1, 36, 16)) == 3
    for name, shape in (("dense.bias", (1,)), ("b0.bn.gamma", (32,)), ("b0.dw0.bias", (32,)), ("stem0.bn.moving_mean", (4,))):
        assert qat.kernel_axis(name, shape) is None


@pytest.mark.parametrize("kind", wq.KINDS)
def test_fake_quant_weights_is_weight_params_per_kernel(kind):
    lay = wq.layout_of(kind)
    ws, vi = wq.crafted_weights(lay)
    fq = qat.fake_quant_weights(lay, ws)
    assert len(fq) == len(ws)
    changed = 0
    for (name, shape, _), w, f in zip(lay.keras_vars, ws, fq):
        assert f.dtype == np.float32 and f.shape == w.shape
        axis = qat.kernel_axis(name, shape)
        if axis is None:
            assert f.tobytes() == w.tobytes(), name
            continue
        q, scale = quantize.weight_params(w, axis)
        bshape = [1] * w.ndim
        bshape[axis] = -1
        assert f.tobytes() == (q.astype(np.float32) * scale.reshape(bshape)).tobytes(), name
        assert np.abs(q).max() <= 127
        # idempotent: the grid's values are on the grid
        assert qat.fake_quant_weights(lay, fq)[len(fq) - 1].tobytes() == fq[-1].tobytes()
        changed += int((f != w).sum())
    assert changed > 0
    k = fq[vi].reshape(-1, ws[vi].shape[3])
    assert k[:6, 2].tolist() == [127.0, 1.0, 2.0, -3.0, 127.0, -127.0] and not k[:, 0].any() and k[2, 3] == 0.0
    # the model form and the packed form agree
    p, s = lay.pack(ws)
    assert qat.forward_params_reference(lay, p, s).tobytes() == lay.pack(fq)[0].tobytes()
    # a channel that is not finite stays as it is
    ws[vi][0, 0, 0, 1] = np.inf
    again = qat.fake_quant_weights(lay, ws)[vi]
    assert again[..., 1].tobytes() == ws[vi][..., 1].tobytes() and again[..., 2].tobytes() == fq[vi][..., 2].tobytes()


def test_fold_bn_keeps_a_channel_grid_up_to_the_sign_of_gamma():
    """per-channel symmetric quantization commutes with a per-channel rescaling: the int8 values of a BN-folded 1x1 kernel are
    the unfolded kernel's, times the sign of gamma (away from float ties)"""
    rng = np.random.default_rng(0)
    kern = rng.normal(0, 0.3, (24, 16)).astype(np.float32)
    gamma = rng.normal(0, 1.0, 16).astype(np.float32)
    var = (0.5 + rng.random(16)).astype(np.float32)
    folded, _ = quantize.fold_bn(kern, gamma, np.zeros(16, np.float32), np.zeros(16, np.float32), var)
    q0, _ = quantize.weight_params(kern, 1)
    q1, _ = quantize.weight_params(folded, 1)
    assert np.mean(q1 == q0 * np.sign(gamma).astype(np.int8)[None, :]) > 0.99


def test_training_config_mapping():
    assert qat.parse_config({}) is None and qat.parse_config({"weight_quantization_aware": None}) is None
    assert qat.parse_config({"weight_quantization_aware": {}}) == {"first_step": 0}
    assert qat.parse_config({"weight_quantization_aware": {"first_step": 7}}) == {"first_step": 7}
    assert qat.parse_config({"weight_quantization_aware": {"first_step": np.int64(3)}}) == {"first_step": 3}
    for bad, word in (({"first_step": -1}, "first_step"), ({"first_step": 1.5}, "first_step"), ({"first_step": "2"}, "first_step"),
                      ({"first_step": True}, "first_step"), ({"first_step": None}, "first_step"), ({"first": 2}, "unknown key first"),
                      (3, "mapping"), ([("first_step", 1)], "mapping")):
        with pytest.raises(ValueError, match="weight_quantization_aware.*" + word):
            qat.parse_config({"weight_quantization_aware": bad})
