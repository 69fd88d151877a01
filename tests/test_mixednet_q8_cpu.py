"""int8 quantization of MixedNets with residual connections or a pooled head without any kernel: the two forms of the NumPy
restatement (tests/quant_mixednet_oracle.py) against each other on every case a kernel test runs, its ADD and its average-pool
rounding against hand-computed values, the quantization contract of microwakeword_amd/quantize_mixednet.py, the input
conditions of every case (``quant_mixednet_checks.conditions``, from the oracle alone) and the early check of the CLI."""
import numpy as np
import pytest

import quant_mixednet_checks as mc
import quant_mixednet_oracle as qmo
from microwakeword_amd import model_train_eval, quantize, quantize_mixednet as qmx, streaming
from microwakeword_amd.layout import GraphMixedNetLayout
import engine_checks as ec


@pytest.mark.parametrize("cid", mc.case_ids())
def test_the_oracle_forms_agree(cid):
    b, qm = mc.built(cid), mc.oracle_model(cid)
    frames = mc.seq_of(cid)[:min(len(mc.seq_of(cid)), (b.desc["t_final"] + 120) * b.s)]
    step = qmo.StepStreamQ8(qm)
    u8, lq = step.run(frames)
    ref_u8, ref_lq, ref_st = qmo.whole_sequence(qm, frames)
    assert np.array_equal(u8, ref_u8) and np.array_equal(lq, ref_lq) and np.array_equal(step.state(), ref_st)
    assert len(np.unique(lq)) > 8
    # past the receptive field, with the stream's outputs ending where the windows end, the non-streaming form is the stream's
    # (stream output j reads the frames from j s - r1 on, conv1 position m of window i those from (i + m) s on: the stream starts
    # o = r1 mod s frames in, and window i ends at stream output i + j0)
    k1 = b.desc["conv1_kernel"]
    r1 = max(0, k1 - b.s)
    o = r1 % b.s
    ns_u8, ns_lq = qmo.non_stream(qm, frames, b.T, want_logits=True)
    st_u8, st_lq, _ = qmo.whole_sequence(qm, frames[o:])
    j0, i0 = (b.T - k1) // b.s + (r1 - o) // b.s, 1
    assert ns_u8.size > i0 + 8
    assert np.array_equal(st_lq[j0 + i0:j0 + ns_lq.size], ns_lq[i0:]) and np.array_equal(st_u8[j0 + i0:j0 + ns_u8.size], ns_u8[i0:])


def test_add_q8_against_hand_computed_values():
    # equal scales, s_out = s: m1 = m2 = 1/2, mo = 2 s / (2^20 s) = 2^-19: ((a + b) 2^19) 2^-19 = a + b exactly
    m = qmo.add_multipliers(0.05, 0.05, 0.05)
    assert m == (1 << 30, 0, 1 << 30, 0, 1 << 30, -18)
    for q1, q2, want in ((10, 20, 30), (-7, 3, -4), (-100, -20, -120), (100, 100, 127), (-100, -100, -128), (0, 0, 0)):
        assert int(qmo.add_q8(q1, 0, q2, 0, m, 0, relu=False)) == want
    assert int(qmo.add_q8(-100, 0, 20, 0, m, 0, relu=True)) == 0            # the fused ReLU: max(-128, zp_out)
    assert int(qmo.add_q8(-100, 0, 20, 0, m, -100, relu=True)) == -100 and int(qmo.add_q8(-100, 0, 20, 0, m, -100, relu=False)) == -128
    assert int(qmo.add_q8(-10, 0, 20, 0, m, -100, relu=True)) == -90
    assert int(qmo.add_q8(13, 5, -2, -3, m, 7, relu=False)) == (13 - 5) + (-2 + 3) + 7   # zero points
    # equal scales, s_out = 2 s: (a + b) / 2, ties away from zero - also for negative sums
    m = qmo.add_multipliers(0.05, 0.05, 0.1)
    for q1, q2, want in ((10, 21, 16), (10, 20, 15), (-10, -21, -16), (-3, 2, -1), (3, -2, 1), (-1, 0, -1), (1, 0, 1)):
        assert int(qmo.add_q8(q1, 0, q2, 0, m, 0, relu=False)) == want, (q1, q2)
    # a 100 : 1 scale ratio (powers of two would hide the multipliers' rounding): real value (100 q1 + q2) s / s_out
    s = 0.001
    m = qmo.add_multipliers(100 * s, s, 100 * s)
    assert m[1] == 0 and m[3] == -7 and m[5] == -18   # m1 = 1/2, m2 = 1/200 = 0.64 x 2^-7, mo = 2^-19
    for q1, q2, want in ((5, 100, 6), (5, 149, 6), (5, 151, 7), (-5, -151, -7), (-5, -149, -6), (-50, 49, -50), (-50, 51, -49), (0, -49, 0)):
        assert int(qmo.add_q8(q1, 0, q2, 0, m, 0, relu=False)) == want, (q1, q2)


def test_average_pool_rounding():
    # positive, negative and tie sums: C's (acc + n / 2) / n and (acc - n / 2) / n, integer n / 2
    for acc, n, want in ((7, 2, 4), (-7, 2, -4), (6, 2, 3), (1, 2, 1), (-1, 2, -1), (0, 2, 0), (12, 5, 2), (13, 5, 3), (-12, 5, -2),
                         (-13, 5, -3), (449, 300, 1), (450, 300, 2), (-449, 300, -1), (-450, 300, -2), (5 * 127, 5, 127), (-128 * 5, 5, -128)):
        assert int(qmo.avg_pool_round(acc, n)) == want, (acc, n)
    assert qmo.avg_pool_round(np.array([7, -7, 0]), 2).tolist() == [4, -4, 0]


def test_tensor_names_with_residuals_on_some_blocks_and_repeats():
    d = mc.vc.desc_of(6, 5, 2, [(2, (3,), 8), (1, (1,), 8), (3, (3, 5), 5)], 3, residual=[1, 0, 1])
    assert qmx.tensor_names(d) == [
        "input", "conv1", "block0.residual", "block0.r0.mixconv", "block0.r0.pointwise", "block0.r0.add", "block0.r1.mixconv",
        "block0.r1.pointwise", "block0.r1.add", "block1.r0.pointwise", "block2.residual", "block2.r0.mixconv", "block2.r0.pointwise",
        "block2.r0.add", "block2.r1.mixconv", "block2.r1.pointwise", "block2.r1.add", "block2.r2.mixconv", "block2.r2.pointwise",
        "block2.r2.add", "dense"]
    plain = {k: v for k, v in d.items() if k != "residual"}
    assert qmx.tensor_names(plain) == quantize.tensor_names(plain)


@pytest.mark.parametrize("blocks,tf", [([(2, (3,), 8), (1, (3, 5), 7), (1, (1,), 6)], 3), ([(1, (3,), 7)], 1)], ids=["multi-kernel", "t_final=1"])
def test_both_quantizers_are_one_on_a_plain_description(blocks, tf):
    """quantize.quantize_weights and quantize_mixednet.quantize_weights are one walk: on a plain description (no residual, no
    head option) they give the same native arrays and the same summary; only the stored ``desc`` differs (as given / normalised)."""
    plain = mc.vc.sw.desc_of(6, 5, 2, blocks, tf)
    general = mc.vc.desc_of(6, 5, 2, blocks, tf)
    lay = GraphMixedNetLayout(mc.vc.flags_of(general), plain["frames"])
    assert lay.t_last == tf
    rng = np.random.default_rng(11)
    ws = [rng.normal(0.0, 0.5, s).astype(np.float32) for _, s, _ in lay.keras_vars]
    ws = [np.abs(w) + np.float32(0.25) if n.endswith(("gamma", "moving_variance")) else w for (n, _, _), w in zip(lay.keras_vars, ws)]
    names = quantize.tensor_names(plain)
    assert names == qmx.tensor_names(general) and len(names) == 3 + sum(r * (1 + (max(ks) > 1)) for r, ks, _ in blocks)
    lo = -rng.random(len(names)) * 4.0
    ranges = np.stack([lo, lo + 0.5 + rng.random(len(names)) * 8.0], 1)
    models = [q.quantize_weights(d, ws, ranges) for q in (quantize, qmx) for d in (plain, general)]
    assert [type(m) for m in models] == [quantize.QuantizedModel] * 2 + [qmx.QuantizedMixedNetModel] * 2
    assert models[0].desc == plain and models[2].desc == models[3].desc == qmx.normalized(general)
    for m in models[1:]:
        for a, b in zip(models[0].packed(), m.packed()):
            assert np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b)
        assert m.summary() == models[0].summary()


def test_quantized_parameters_follow_the_contract():
    cid = "res-consecutive_cin-eq-f_rep3_nodw_g2_s1-k1eq_avg-tf2"
    b, qm = mc.built(cid), mc.oracle_model(cid)
    at = {n: t for t, n in enumerate(qm.names)}
    kinds = [op["kind"] for op in qm.ops]
    assert kinds[0] == "conv1" and kinds[-1] == "dense" and kinds.count("res") == 3 and kinds.count("pw_add") == 5
    assert qm.ops[-1]["weights"].shape == (1, 7)                      # a pooled Dense reads the C pooled values
    t_in = 1
    for op in qm.ops[1:-1]:
        assert op["tensors"][0] == t_in                                # a residual is kept aside; an ADD output feeds the next layer
        if op["kind"] == "pw_add":
            t1, t2, to = op["add_tensors"]
            assert qm.names[t1].endswith(".pointwise") and qm.names[t2].endswith(".residual") and qm.names[to].endswith(".add")
            assert op["add"].tolist() == list(qmo.add_multipliers(qm.scales[t1], qm.scales[t2], qm.scales[to]))
            assert all(sh <= 0 for sh in op["add"][1::2])
            t_in = to
        elif op["kind"] != "res":
            t_in = op["tensors"][1]
    # block 0, repeat 1: its MixConv reads repeat 0's ADD output
    mix1 = next(op for op in qm.ops if op["tensors"][1] == at["block0.r1.mixconv"])
    assert mix1["tensors"][0] == at["block0.r0.add"]
    wq, iv, s0, lut = qm.packed()
    assert iv.size == 3 * sum(op["bias"].size for op in qm.ops) + 6 * 5 + len(qm.names)
    assert np.array_equal(iv[-len(qm.names):], qm.zero_points) and s0 == qm.scales[0]
    assert np.array_equal(lut, quantize.logistic_table(qm.scales[-1], qm.zero_points[-1]))
    # a residual op: [Co][r4(Ci)], bias with its input zero point folded
    r0 = qm.ops[1]
    ci, co = r0["weights"].shape
    n0 = qm.ops[0]["weights"].size
    assert r0["kind"] == "res" and np.array_equal(wq[n0:n0 + co * ci].reshape(co, ci), r0["weights"].T)
    c1 = qm.ops[0]["bias"].size
    assert np.array_equal(iv[3 * c1:3 * c1 + co], r0["bias"].astype(np.int64) - int(qm.zero_points[1]) * r0["weights"].astype(np.int64).sum(axis=0))
    with pytest.raises(ValueError, match="calibrated ranges"):
        qmx.quantize_weights(mc.desc_of(b), b.weights, qm.ranges[:-1])
    with pytest.raises(ValueError, match="more weights"):
        qmx.quantize_weights(mc.desc_of(b), list(b.weights) + [np.zeros(1)], qm.ranges)


def test_an_add_output_multiplier_of_one_or_more_is_refused_naming_the_tensor():
    cid = "max-tf2_res"
    b, qm = mc.built(cid), mc.oracle_model(cid)
    ranges = np.array(qm.ranges, np.float64)
    t = qm.names.index("block0.r0.add")
    ranges[t] = (0.0, ranges[qm.names.index("block0.residual"), 1] * 2e-6)   # s_out < 2 max(s1, s2) / 2^20
    with pytest.raises(ValueError, match=r"block0\.r0\.add.*not below one"):
        qmx.quantize_weights(mc.desc_of(b), b.weights, ranges)


def test_npz_round_trip_and_load_quantized_dispatch(tmp_path):
    cid = "res-first-last_cin-ne-f_rep2_s2-k1gt_tf3"
    qm = mc.oracle_model(cid)
    path = str(tmp_path / "q.npz")
    qm.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert str(z["family"]) == "mixednet_variant"
    back = streaming.load_quantized(path)
    assert isinstance(back, qmx.QuantizedMixedNetModel) and back.desc == qm.desc and back.names == qm.names
    for a, c in zip(qm.packed(), back.packed()):
        assert np.array_equal(a, c)
    assert back.summary() == qm.summary() and "block0.r1.add" in qm.summary()
    frames = mc.seq_of(cid)[:120]
    for a, c in zip(qmo.whole_sequence(qm, frames), qmo.whole_sequence(back, frames)):
        assert np.array_equal(a, c)
    plain = mc.qc.synthetic_quantized(dict(conv1_filters=8, conv1_kernel=3, stride=1, blocks=[(1, (3,), 8)], t_final=4, frames=20))
    plain.save(str(tmp_path / "m.npz"))
    assert isinstance(streaming.load_quantized(str(tmp_path / "m.npz")), quantize.QuantizedModel)
    with pytest.raises(ValueError, match="not a residual / pooled MixedNet file"):
        qmx.QuantizedMixedNetModel.load(str(tmp_path / "m.npz"))


@pytest.mark.parametrize("cid", mc.case_ids())
def test_every_kernel_case_meets_the_input_conditions(cid):
    fig = mc.conditions(mc.oracle_model(cid), mc.seq_of(cid), cid)
    print("[mixednet_q8] %s: distinct logits %d, most frequent %.3f, clamped %.3f, ADDs (distinct 1x1, distinct r, clamped) %s" % (
        cid, fig["distinct"], fig["share"], fig["clamped"], fig["adds"]))


def test_the_average_pool_cases_see_both_signs_and_exact_ties():
    pos = neg = ties = 0
    for cid in mc.case_ids():
        qm = mc.oracle_model(cid)
        if qm.desc["pool"] != "average":
            continue
        tf = qm.desc["t_final"]
        for acc in mc.conditions(qm, mc.seq_of(cid), cid)["pool_acc"]:
            pos, neg = pos + int((acc > 0).sum()), neg + int((acc < 0).sum())
            ties += int(((2 * np.abs(acc)) % (2 * tf) == tf).sum())   # |acc| / T_f has the fraction 1/2 exactly
    print("[mixednet_q8] average-pool accumulators: %d positive, %d negative, %d exact ties" % (pos, neg, ties))
    assert pos > 0 and neg > 0 and ties > 0


def test_the_relu_clamp_case_cuts_values_the_int8_floor_would_keep():
    qm = mc.oracle_model("relu-clamp")
    adds = []
    qmo.whole_sequence(qm, mc.seq_of("relu-clamp"), add_trace=adds)
    assert adds
    for q1, r, out, zo, z1, z2, mult in adds:
        assert zo > -128
        assert np.any(qmo.add_q8(q1, z1, r, z2, mult, zo, relu=False) < zo) and out.min() == zo


def test_the_add_rounding_case_tells_the_rounding_of_the_scaled_inputs():
    qm = mc.oracle_model("add-rounding")
    t = {n: i for i, n in enumerate(qm.names)}
    assert [float(qm.scales[t["block0.r0." + n]]) for n in ("pointwise", "add")] + [float(qm.scales[t["block0.residual"]])] == [7 / 64, 1 / 64, 1.5 / 64]
    adds = []
    qmo.whole_sequence(qm, mc.seq_of("add-rounding"), add_trace=adds)
    for q1, r, out, zo, z1, z2, mult in adds:
        n = int(np.sum(qmo.add_q8(q1, z1, r, z2, mult, zo, input_rounding=False) != out))
        print("[mixednet_q8] add-rounding: %d of %d ADD outputs depend on the rounding of the scaled inputs" % (n, out.size))
        assert n >= 32


def test_the_tiles_of_the_three_placements():
    assert mc.tile_bytes(mc.case("wide-scratch").desc) > 160 * 1024
    assert 64 * 1024 < mc.tile_bytes(mc.case("default48").desc) <= 160 * 1024
    assert all(mc.tile_bytes(mc.case(c).desc) <= 64 * 1024 for c in mc.case_ids() if c not in ("wide-scratch", "default48"))



class _NoDevice:
    """a model whose device side must not be touched"""

    def __init__(self, flags):
        self.flags = flags
        self.layout = GraphMixedNetLayout(flags, 52)

    def __getattr__(self, name):
        raise AssertionError("the refusal must come before the model's %s is used" % name)


@pytest.mark.parametrize("bad,name", [(dict(spatial_attention=1), "spatial_attention"), (dict(first_conv_filters=0), "first_conv_filters = 0")])
def test_the_module_refuses_before_any_device_work(bad, name):
    model = _NoDevice(dict(ec.DEF, residual_connection="1,0,1,0", **bad))
    with pytest.raises(NotImplementedError, match=name):
        qmx.calibrate(model, None, {"stride": 1, "spectrogram_length": 52})
    with pytest.raises(NotImplementedError, match=name):
        qmx.quantize(model, np.zeros((4, 2), np.float32))


def test_the_plain_module_names_this_one():
    model = _NoDevice(dict(ec.DEF, residual_connection="1,0,1,0"))
    with pytest.raises(NotImplementedError, match="residual_connection.*quantize_mixednet"):
        quantize.calibrate(model, None, {"stride": 1, "spectrogram_length": 52})


def _config_file(tmp_path):
    import yaml
    cfg = {"train_dir": str(tmp_path / "run"), "clip_duration_ms": 1500, "batch_size": 8, "features": []}
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.dump(cfg))
    return str(path), tmp_path / "run"


def test_native_ext_lets_residual_and_pooled_through_the_early_check(tmp_path):
    path, _ = _config_file(tmp_path)
    for extra in (["--residual_connection", "1,0,1,0"], ["--residual_connection", "0,0,0,0", "--pooled", "1"],
                  ["--residual_connection", "1,0,1,0", "--pooled", "1", "--max_pool", "1"], ["--residual_connection", "0,0,0,0"]):
        flags = model_train_eval.build_parser().parse_args(
            ["--training_config", path, "--test_tflite_streaming_quantized", "1", "--quantized_backend", "native_ext", "mixednet"] + extra)
        model_train_eval.check_evaluation_flags(flags, model_train_eval.mixednet, model_train_eval.load_config(flags, model_train_eval.mixednet))
    # the keyword is off by default: native still refuses, and names the way in
    with pytest.raises(NotImplementedError, match="residual_connection.*native_ext"):
        streaming.check_evaluation_topology(dict(ec.DEF, residual_connection="1,0,1,0"), 52, 1, [], int8=True)
    streaming.check_evaluation_topology(dict(ec.DEF, residual_connection="1,0,1,0"), 52, 1, [], int8=True, int8_variants=True)


@pytest.mark.parametrize("argv,name", [
    (["--residual_connection", "1,0,1,0", "--spatial_attention", "1"], "spatial_attention"),
    (["--residual_connection", "0,0,0,0", "--pooled", "1", "--spatial_attention", "1"], "spatial_attention"),
    (["--residual_connection", "1,0,1,0", "--first_conv_filters", "0"], "first_conv_filters = 0"),
])
def test_native_ext_still_refuses_before_training(tmp_path, monkeypatch, argv, name):
    path, run = _config_file(tmp_path)

    def no_model(*a, **k):
        raise AssertionError("the topology check must run before the model is built")
    monkeypatch.setattr(model_train_eval.mixednet, "model", no_model)
    with pytest.raises(NotImplementedError, match=name):
        model_train_eval.main(["--training_config", path, "--train", "1", "--test_tflite_streaming_quantized", "1", "--quantized_backend",
                               "native_ext", "mixednet"] + argv)
    assert not run.exists()


def test_native_ext_takes_the_plain_path_for_a_plain_model_and_for_inception():
    from microwakeword_amd import quantize_graph
    from microwakeword_amd.layout import InceptionLayout

    class _M:
        def __init__(self, flags, layout=None):
            self.flags, self.layout = flags, layout
    plain, variant = _M(dict(ec.DEF)), _M(dict(ec.DEF, residual_connection="1,0,1,0"))
    assert model_train_eval.quantization_module(plain, "native_ext") is quantize
    assert model_train_eval.quantization_module(plain, "native") is quantize
    assert model_train_eval.quantization_module(variant, "native_ext") is qmx
    assert model_train_eval.quantization_module(_M(dict(ec.DEF, pooled=1)), "native_ext") is qmx
    assert model_train_eval.quantization_module(variant, "native") is quantize   # whose refusal then names native_ext's module
    inc = _M({}, object.__new__(InceptionLayout))
    assert model_train_eval.quantization_module(inc, "native_ext") is quantize_graph
