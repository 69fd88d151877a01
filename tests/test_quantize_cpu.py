"""Host side of the int8 streaming model (microwakeword_amd/quantize.py): TFLite's fixed-point helpers on known answers,
activation / weight / bias parameters, BN folding, the logistic table, the .npz round trip, the calibration draw, and
that the gfx950 build of the int8 kernel really runs on the integer dot-product instructions."""
import os
import re
import subprocess

import numpy as np
import pytest

import quant_oracle as qo
from microwakeword_amd import quantize as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantize_multiplier_known_answers():
    assert q.quantize_multiplier(0.5) == (1 << 30, 0)
    assert q.quantize_multiplier(0.0123456789) == (1696777188, -6)
    assert q.quantize_multiplier(0.0) == (0, 0)
    assert q.quantize_multiplier(1.0) == (1 << 30, 1)
    assert q.quantize_multiplier(2.0 ** -40) == (0, 0)                    # shift < -31
    M, sh = q.quantize_multiplier(1.0 - 2.0 ** -40)                       # rounds up to 2^31: halved, shift + 1
    assert (M, sh) == (1 << 30, 1)


def test_srdhm_rdpot_mbqm_known_answers():
    M, sh = q.quantize_multiplier(0.0123456789)
    for x, want in ((1000, 12), (-1000, -12), (40500, 500), (-40500, -500)):
        assert q.mbqm(x, M, sh) == want
        assert int(qo.mbqm(x, M, sh)) == want
    assert q.rdpot(3, 1) == 2 and q.rdpot(-3, 1) == -2
    assert q.rdpot(5, 1) == 3 and q.rdpot(-5, 1) == -3 and q.rdpot(4, 2) == 1 and q.rdpot(-6, 2) == -2   # ties away from 0
    assert q.rdpot(7, 0) == 7
    assert q.srdhm(q.INT32_MIN, q.INT32_MIN) == q.INT32_MAX
    assert q.srdhm(1 << 30, 1 << 30) == 1 << 29
    assert q.srdhm(-(1 << 30), 1 << 30) == -(1 << 29)
    assert q.srdhm(1, 1 << 30) == 1 and q.srdhm(-1, 1 << 30) == 0          # +-0.5: nudge 2^30 vs 1 - 2^30, truncation
    rng = np.random.default_rng(0)
    a = rng.integers(q.INT32_MIN, q.INT32_MAX, 2000)
    b = rng.integers(0, q.INT32_MAX, 2000)
    e = rng.integers(0, 32, 2000)
    assert np.array_equal(qo.srdhm(a, b), [q.srdhm(int(x), int(y)) for x, y in zip(a, b)])
    assert np.array_equal(qo.rdpot(a, e), [q.rdpot(int(x), int(k)) for x, k in zip(a, e)])
    sh = rng.integers(-31, 4, 2000)
    assert np.array_equal(qo.mbqm(a >> 8, b, sh), [q.mbqm(int(x) >> 8, int(y), int(s)) for x, y, s in zip(a, b, sh)])


def test_activation_params():
    assert q.activation_params(0.0, 0.0) == (np.float32(1.0), 0)
    s, z = q.activation_params(0.0, 26.0)                                 # one-sided: the input's [0, >= 26]
    assert s == np.float32(26.0 / 255) and z == -128
    s, z = q.activation_params(-3.0, 0.0)
    assert s == np.float32(3.0 / 255) and z == 127
    s, z = q.activation_params(2.0, 5.0)                                  # widened to hold zero
    assert s == np.float32(5.0 / 255) and z == -128
    s, z = q.activation_params(-1.0, 1.0)
    assert s == np.float32(2.0 / 255) and z == -1                         # zp -0.5 rounds away from zero
    s, z = q.activation_params(-1.0, 3.0)
    assert z == -64                                                       # -128 + 63.75 -> -64.25 -> -64
    assert q.round_half_away(-0.5) == -1 and q.round_half_away(2.5) == 3


def test_weights_bias_and_bn_fold():
    w = np.array([[0.5, 0.0, -2.0], [-1.0, 0.0, 1.0]], np.float32)         # [Ci, Co], per output channel (axis 1)
    qw, sc = q.weight_params(w, 1)
    assert np.array_equal(sc, np.array([1.0 / 127, 1.0, 2.0 / 127], np.float32))
    assert np.array_equal(qw, np.array([[64, 0, -127], [-127, 0, 64]], np.int8))   # 63.5 -> 64 (ties away)
    assert np.array_equal(q.bias_q([0.25, -0.25, 1.0], np.float32(0.5), [0.25, 0.5, 1e-3]), [2, -1, 2000])
    kern = np.array([[1.0, 2.0]], np.float32)
    fw, fb = q.fold_bn(kern, [2.0, 1.0], [0.5, 0.0], [1.0, -1.0], [3.999, 0.999])
    assert np.allclose(fw, [[1.0, 2.0]]) and np.allclose(fb, [-0.5, 1.0])
    assert fw.dtype == np.float32 and fb.dtype == np.float32


def test_logistic_table():
    lut = q.logistic_table(np.float32(0.1), -10)
    assert lut.dtype == np.uint8 and lut.size == 256
    assert np.all(np.diff(lut.astype(np.int32)) >= 0)
    assert lut[0] == 0 and lut[-1] == 255                                 # sigmoid(-11.8) * 256 rounds to 0, sigmoid(13.7) to 256 -> 255
    assert lut[-10 + 128] == 128                                          # logit 0 -> 0.5
    flat = q.logistic_table(np.float32(1e-6), 0)
    assert np.all(flat == 128)


def _tiny_desc():
    return dict(conv1_filters=4, conv1_kernel=3, stride=1, blocks=[(1, (3,), 5), (1, (1,), 6)], t_final=2, frames=7, mode="stream")


def _tiny_weights(rng):
    d = _tiny_desc()
    return [rng.normal(0, 0.3, (3, 1, 40, 4)), rng.normal(0, 0.3, (3, 1, 4, 1)), rng.normal(0, 0.1, 4),
            rng.normal(0, 0.3, (1, 1, 4, 5)), 1 + rng.random(5), rng.normal(0, 0.1, 5), rng.normal(0, 0.1, 5), 1 + rng.random(5),
            rng.normal(0, 0.3, (1, 1, 5, 6)), 1 + rng.random(6), rng.normal(0, 0.1, 6), rng.normal(0, 0.1, 6), 1 + rng.random(6),
            rng.normal(0, 0.3, (d["t_final"] * 6, 1)), rng.normal(0, 0.1, 1)]


def test_quantize_weights_and_npz_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    desc = _tiny_desc()
    names = q.tensor_names(desc)
    assert names == ["input", "conv1", "block0.r0.mixconv", "block0.r0.pointwise", "block1.r0.pointwise", "dense"]
    ranges = np.array([[0, 26], [0, 3], [-2, 2], [0, 4], [0, 1], [-6, 5]], np.float32)
    qm = q.quantize_weights(desc, _tiny_weights(rng), ranges)
    assert [op["kind"] for op in qm.ops] == ["conv1", "mix", "pw", "pw", "dense"]
    assert qm.zero_points[0] == -128 and qm.zero_points[1] == -128
    assert np.array_equal(qm.ops[0]["bias"], np.zeros(4, np.int32))      # conv1 has no bias
    w, iv, s_in, lut = qm.packed()
    assert w.size % 4 == 0 and s_in == qm.scales[0] and lut.size == 256
    path = str(tmp_path / "m.npz")
    qm.save(path)
    with np.load(path, allow_pickle=False) as z:                         # data only
        assert all(z[k].dtype != object for k in z.files)
    back = q.QuantizedModel.load(path)
    for a, b in zip(qm.packed(), back.packed()):
        assert np.array_equal(a, b)
    assert back.desc == json_round(desc) and back.names == names
    assert np.array_equal(back.ranges, ranges)
    text = back.summary()
    assert "block0.r0.mixconv" in text and "zero_point" in text
    with pytest.raises(ValueError, match="calibrated ranges"):
        q.quantize_weights(desc, _tiny_weights(rng), ranges[:-1])


def json_round(d):
    import json
    return json.loads(json.dumps(d))


class RecordingProcessor:
    def __init__(self, n, L):
        self.calls = []
        self.x = np.random.default_rng(2).uniform(1, 20, size=(n, L, 40)).astype(np.float32)

    def get_data(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.x.copy(), np.zeros(self.x.shape[0]), np.ones(self.x.shape[0])


def test_calibration_draws_once_and_fixes_two_pixels():
    L, s = 8, 2
    dp = RecordingProcessor(500, L)
    frames = q.calibration_frames(dp, {"spectrogram_length": L, "stride": s})
    assert dp.calls == [(("training", 500), {"features_length": L})]
    n = len(range(0, L - s, s))
    assert frames.shape == (500 * n * s, 40) and frames.dtype == np.float32
    assert frames[0, 0] == 0.0 and frames[0, 1] == 26.0
    want = dp.x.copy()
    want[0][0, 0], want[0][0, 1] = 0.0, 26.0
    assert np.array_equal(frames, want[:, :n * s].reshape(-1, 40))


def test_calibrate_runs_the_float_stream_once(emu_lib):
    import engine_checks as ec
    import streaming_checks as sc
    _, model = sc.make_model(emu_lib, ec.DEF, 52)
    dp = RecordingProcessor(500, 4)
    ranges = q.calibrate(model, dp, {"spectrogram_length": 4, "stride": 1})
    assert len(dp.calls) == 1
    assert ranges.shape == (len(q.tensor_names(sc.streaming.StreamingModel(model, 1).desc)), 2)
    assert ranges[0, 0] == 0.0 and ranges[0, 1] == 26.0
    qm = q.quantize(model, ranges)
    assert qm.zero_points[0] == -128


def test_gfx950_build_runs_int8_dot_products(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.isfile(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "q8.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "--cuda-device-only", "-S",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "microwakeword_amd", "csrc", "tu_stream_q8.hip"),
                    "-o", out], check=True)
    asm = open(out).read()
    for var in ("Lb0E", "Lb1E"):   # stream_q8_kernel<false> (a plain plan) and <true> (residuals / a pooled head)
        m = re.search(r"^(_Z\w*stream_q8_kernelI%s\w*):" % var, asm, re.M)
        assert m, "stream_q8_kernel<%s> not found in the gfx950 assembly" % var
        body = asm[m.end():asm.index(".size\t" + m.group(1), m.end())]
        assert re.search(r"\bv_dot4c?_i32_i8|\bv_mfma_i32_16x16x64_i8", body), "no int8 dot / MFMA instruction in the int8 kernel <%s>" % var
