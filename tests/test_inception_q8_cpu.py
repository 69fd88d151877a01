"""int8 quantization of Inception models without any kernel: the quantization contract of
microwakeword_amd/quantize_graph.py, the two forms of the NumPy restatement (tests/quant_graph_oracle.py) against each
other, and the input condition (``q8_checks.SPREAD_*``, from the oracle alone) of every case a kernel test runs."""
import os
import re
import subprocess

import numpy as np
import pytest

import engine_checks as ec
import q8_checks as qc
import quant_graph_checks as gc
import quant_graph_oracle as qgo
from microwakeword_amd import quantize, quantize_graph, streaming


def _names(qm):
    return {n: t for t, n in enumerate(qm.names)}


def test_concatenation_classes_of_the_default_flags_are_b1_b2b_b3c_per_block():
    qm = gc.cases()["emu/INC"].qm
    at = _names(qm)
    groups = {}
    for t, c in enumerate(qm.classes):
        groups.setdefault(c, []).append(t)
    multi = sorted(sorted(g) for g in groups.values() if len(g) > 1)
    want = sorted(sorted(at["i%d.%s" % (b, n)] for n in ("b1", "b2b", "b3c")) for b in range(3))
    assert multi == want
    for g in multi:
        assert len({float(qm.scales[t]) for t in g}) == 1 and len({int(qm.zero_points[t]) for t in g}) == 1
        lo, hi = qm.ranges[g, 0].min(), qm.ranges[g, 1].max()
        assert (qm.scales[g[0]], qm.zero_points[g[0]]) == quantize.activation_params(lo, hi)
        assert any(quantize.activation_params(*qm.ranges[t]) != (qm.scales[t], qm.zero_points[t]) for t in g), \
            "the members' own ranges give the class parameters: this case cannot tell a class from a tensor"
    # every op reads one (scale, zero point), whatever its sources
    for srcs in qm.sources:
        assert len({(float(qm.scales[t]), int(qm.zero_points[t])) for t, _, _ in srcs}) == 1


def test_a_tensor_feeding_two_concatenations_merges_them_and_the_input_joins_like_any_tensor():
    ops = [dict(src=[-1], kernel=1, filters=8), dict(src=[-1], kernel=1, filters=8), dict(src=[0], kernel=1, filters=8),
           dict(src=[0, 1], kernel=1, filters=8), dict(src=[1, 2], kernel=1, filters=8), dict(src=[-1, 4], kernel=1, filters=8)]
    cls = quantize_graph.concat_classes(dict(conv_ops=ops))
    # tensors: 0 input, 1 + i.  {1, 2} and {2, 3} share tensor 2; {0, 5} holds the input; tensors 4 and 6 stand alone
    assert cls == [0, 1, 1, 1, 4, 0, 6]


def test_fold_weights_bias_multiplier_and_packed_layout():
    case = gc.cases()["emu/INC_VARIANT"]
    desc, w, qm, om = case.build()
    it = iter(w)
    for i, (o, srcs, op) in enumerate(zip(desc["conv_ops"], qm.sources, qm.ops)):
        kern, gamma, beta, mean, var = (np.asarray(next(it), np.float64) for _ in range(5))
        k, co, g = o["kernel"], o["filters"], o["bn_groups"]
        slot = np.arange(co) % g if g > 1 else np.arange(co)
        sc = gamma[slot] / np.sqrt(var[slot] + 1e-3)
        fw = (kern.reshape(k, -1, co) * sc).astype(np.float32)
        fb = (beta[slot] - mean[slot] * sc).astype(np.float32)
        amax = np.abs(fw.astype(np.float64)).max(axis=(0, 1))
        assert np.array_equal(op["weight_scales"], (amax / 127.0).astype(np.float32))
        assert np.abs(op["weights"].astype(np.int64)).max(axis=(0, 1)).tolist() == [127] * co
        s_in, s_out = np.float64(qm.scales[srcs[0][0]]), np.float64(qm.scales[1 + i])
        assert np.array_equal(op["bias"], quantize.bias_q(fb, qm.scales[srcs[0][0]], op["weight_scales"]))
        m = [quantize.quantize_multiplier(s_in * np.float64(sw) / s_out) for sw in op["weight_scales"]]
        assert op["multiplier"].tolist() == [a for a, _ in m] and op["shift"].tolist() == [b for _, b in m]
    wq, iv, s0, lut = qm.packed()
    kp = lambda srcs: sum((cn + 3) & ~3 for _, _, cn in srcs)   # noqa: E731
    assert wq.size == sum(o["filters"] * o["kernel"] * kp(s) for o, s in zip(desc["conv_ops"], qm.sources)) + \
        qm.ops[-1]["weights"].shape[0] * ((qm.ops[-1]["weights"].shape[1] + 3) & ~3)
    assert iv.size == 3 * sum(o["filters"] for o in desc["conv_ops"]) + 3 + len(desc["conv_ops"]) + 2
    assert np.array_equal(iv[-(len(desc["conv_ops"]) + 2):], qm.zero_points) and s0 == qm.scales[0]
    # op 0: [Co][k][r4(40)] output-major, bias with the input zero point folded
    op0 = qm.ops[0]
    k, ci, co = op0["weights"].shape
    assert np.array_equal(wq[:co * k * ci].reshape(co, k, ci), op0["weights"].transpose(2, 0, 1))
    assert np.array_equal(iv[:co], op0["bias"].astype(np.int64) - int(qm.zero_points[0]) * op0["weights"].astype(np.int64).sum(axis=(0, 1)))
    assert np.array_equal(lut, quantize.logistic_table(qm.scales[-1], qm.zero_points[-1]))


def test_padding_entries_of_a_slice_are_zero_and_every_op_starts_on_a_word():
    qm = gc.cases()["emu/FUSED_10"].qm
    wq = qm.packed()[0]
    at = 0
    for o, srcs, op in zip(qm.desc["conv_ops"], qm.sources, qm.ops):
        assert at % 4 == 0
        co, k = o["filters"], o["kernel"]
        kp = sum((cn + 3) & ~3 for _, _, cn in srcs)
        blk = wq[at:at + co * k * kp].reshape(co, k, kp)
        col = c = 0
        for _, _, cn in srcs:
            assert np.array_equal(blk[:, :, col:col + cn], op["weights"][:, c:c + cn].transpose(2, 0, 1))
            assert not blk[:, :, col + cn:col + ((cn + 3) & ~3)].any()
            col, c = col + ((cn + 3) & ~3), c + cn
        at += blk.size


def test_npz_round_trip_and_family_key(tmp_path):
    qm = gc.cases()["emu/INC"].qm
    path = str(tmp_path / "q.npz")
    qm.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert str(z["family"]) == "graph"
    back = streaming.load_quantized(path)
    assert isinstance(back, quantize_graph.QuantizedGraphModel) and back.desc == qm.desc
    for a, b in zip(qm.packed(), back.packed()):
        assert np.array_equal(a, b)
    assert back.summary() == qm.summary() and "i0.b2b" in qm.summary()
    frames = qc.calibration_set(90, 3)
    for a, b in zip(qgo.whole_sequence(qm, frames), qgo.whole_sequence(back, frames)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="MixedNet file"):
        mixed = qc.synthetic_quantized(dict(conv1_filters=8, conv1_kernel=3, stride=1, blocks=[(1, (3,), 8)], t_final=4, frames=20))
        mixed.save(str(tmp_path / "m.npz"))
        quantize_graph.QuantizedGraphModel.load(str(tmp_path / "m.npz"))
    assert isinstance(streaming.load_quantized(str(tmp_path / "m.npz")), quantize.QuantizedModel)


def test_quantize_weights_refuses_wrong_ranges_and_weights():
    desc, w, qm, _ = gc.cases()["emu/INC"].build()
    with pytest.raises(ValueError, match="calibrated ranges"):
        quantize_graph.quantize_weights(desc, w, qm.ranges[:-1])
    bad = qm.ranges.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        quantize_graph.quantize_weights(desc, w, bad)
    with pytest.raises(ValueError, match="more weights"):
        quantize_graph.quantize_weights(desc, list(w) + [np.zeros(1)], qm.ranges)


@pytest.mark.parametrize("name", ["emu/INC", "emu/INC_VARIANT", "emu/RANDOM_3", "emu/FUSED_10", "emu/FUSED_16"])
def test_step_oracle_equals_whole_sequence_oracle(name):
    case = gc.cases()[name]
    frames = case.frames()[:150]
    step = qgo.StepStreamQ8(case.qm)
    u8, lq = step.run(frames)
    ref_u8, ref_lq, ref_st = qgo.whole_sequence(case.qm, frames)
    assert np.array_equal(u8, ref_u8) and np.array_equal(lq, ref_lq) and np.array_equal(step.state(), ref_st)
    assert len(np.unique(lq)) > 8
    # past the receptive field the non-streaming windows are the stream's outputs
    ns = qgo.non_stream(case.qm, frames, case.T)
    assert np.array_equal(ns, ref_u8[case.T - 1:])


def test_float64_restatements_agree():
    case = gc.cases()["emu/INC_VARIANT"]
    desc, w, _, om = case.build()
    frames = qc.calibration_set(120, 5)
    a, b = gc.float64_ranges(om, case.flags, frames), gc.desc_ranges(desc, w, frames)
    assert np.all(np.abs(a - b) <= 1e-5 * np.abs(a).max(axis=1, keepdims=True))   # desc_ranges folds to float32 first


@pytest.mark.parametrize("name", sorted(gc.cases()))
def test_every_kernel_case_meets_the_input_condition(name):
    case = gc.cases()[name]
    print("[inception_q8] %s spread (distinct logits, most frequent share, clamped share) %s" % (
        name, gc.check_spread(case.qm, case.frames(), name)))


def test_the_relu_case_has_zero_points_above_the_int8_floor_and_accumulators_below_them():
    case = gc.cases()["emu/RELU_ZP"]
    qm = case.qm
    assert all(int(z) > -128 for z in qm.zero_points[1:-1])
    trace = []
    qgo.whole_sequence(qm, case.frames(), trace=trace)
    assert all(np.any(a == zp) and a.min() == zp for _, zp, a in trace)   # the clamp is hit, and nothing lies below it


def test_the_random_topologies_cover_the_axes():
    flags = [ec.random_inception_flags(i) for i in gc.SWEEP]
    ints = lambda f, k: [int(v) for v in str(f[k]).split(",")]   # noqa: E731
    assert len(flags) >= 8
    assert any(len(ints(f, "cnn1_filters")) == 2 for f in flags)
    assert any(2 in ints(f, "cnn2_dilation") for f in flags)
    assert any(max(ints(f, "cnn1_subspectral_groups")) > 1 for f in flags)
    assert any(max(ints(f, "cnn2_subspectral_groups")) > 1 for f in flags)


def test_gfx950_build_of_the_int8_graph_kernel_runs_dot_products_without_scratch(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.isfile(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "gq8.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "--cuda-device-only", "-S",
                    "-I", os.path.join(root, "include"), os.path.join(root, "microwakeword_amd", "csrc", "tu_stream_graph_q8.hip"),
                    "-o", out], check=True)
    asm = open(out).read()
    m = re.search(r"^(_Z\w*stream_graph_q8_kernel\w*):", asm, re.M)
    assert m, "stream_graph_q8_kernel not found in the gfx950 assembly"
    end = asm.index(".amdhsa_kernel " + m.group(1), m.end())   # the kernel descriptor follows the code
    assert re.search(r"\bv_dot4c?_i32_i8", asm[m.end():end]), "no int8 dot instruction in the int8 graph kernel"
    meta = asm[end:asm.index(".end_amdhsa_kernel", end)]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "the int8 graph kernel uses scratch"


def test_synthetic_quantized_serves_descriptions_no_float_model_instantiates():
    desc = gc.fused_description(10, 40)
    qm = qgo.synthetic_quantized(desc, seed=3)
    assert len(qm.ops) == len(desc["conv_ops"]) + 1 and qm.ops[-1]["weights"].shape == (qgo.final_frames(desc), 12)
    assert any(c0 % 4 for srcs in qm.sources for _, c0, _ in srcs)
    frames = qc.calibration_set(70, 2)
    u8, lq = qgo.StepStreamQ8(qm).run(frames)
    ref = qgo.whole_sequence(qm, frames)
    assert np.array_equal(u8, ref[0]) and np.array_equal(lq, ref[1])
