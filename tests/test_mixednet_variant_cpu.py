"""CPU side of the streaming evaluation of residual / pooled / attention MixedNets: the new oracle against itself and against
the non-streaming oracle the reference-graph fixture pins, the conditions on the inputs of tests/mixednet_variant_checks.py,
the coverage of its case list, the description function and the refusals that must come before any device work."""
import numpy as np
import pytest

import engine_checks as ec
import mixednet_variant_checks as vc
import mixednet_variant_streaming_oracle as vo
import streaming_checks as sc
import streaming_oracle as so
from microwakeword_amd import model_train_eval, quantize, streaming
from microwakeword_amd.layout import GraphMixedNetLayout

STREAM_IDS = [cid for cid in vc.case_ids() if not vc.case(cid).desc["attention"]]


def test_the_case_list_covers_every_required_item():
    assert vc.uncovered() == []
    for c in vc.cases():
        assert max([c.desc["conv1_filters"]] + [f for _, _, f in c.desc["blocks"]]) <= 16, c.id


@pytest.mark.parametrize("cid", vc.case_ids())
def test_float32_restatement_within_a_quarter_of_the_bounds(cid):
    ratios = vc.float32_condition(cid)
    print("[mixednet_variant] %s float32 / float64: logits %.3f FWD_TOL, probabilities %.3f PROB_TOL, rings %.3f FWD_TOL" % ((cid,) + ratios))
    assert max(ratios) <= 0.25, (cid, ratios)


@pytest.mark.parametrize("cid", STREAM_IDS)
def test_step_form_equals_whole_sequence_form(cid):
    b = vc.built(cid)
    frames = b.seq[:(max(b.net.ring_sizes()) + 40) * b.s + (b.s - 1)]
    step = vo.StepStream(b.net)
    z_step = step.run(frames)
    z, st = vo.whole_sequence(b.net, frames, rings=True)
    assert z.shape == z_step.shape and np.abs(z - z_step).max() <= 1e-9
    assert np.abs(st - step.state()).max() <= 1e-9
    # and part of the way: the rings of a cold stream
    n = 3 * b.s
    step = vo.StepStream(b.net)
    step.run(frames[:n])
    assert np.abs(vo.whole_sequence(b.net, frames[:n], rings=True)[1] - step.state()).max() <= 1e-9


# residual, pooled average, pooled max, residual + pooled (and every other stream case): once T frames have been fed the
# stream logit at a stride-aligned frame is the non-streaming oracle - the graph ref_graph_golden.npz pins - on the window
# ending there
@pytest.mark.parametrize("cid", STREAM_IDS)
def test_warm_stream_equals_the_non_streaming_oracle(cid):
    b = vc.built(cid)
    T, s = b.T, b.s
    k1 = b.desc["conv1_kernel"]
    frames = b.seq[:T + 23 * s].astype(np.float64)
    z = vo.whole_sequence(b.net, frames)
    checked = 0
    assert (T - k1) % s == 0   # the window's last conv1 output reads its last frame
    for n in range(z.size):
        e = n * s + min(k1, s)   # one past the last frame output n reads: (n + 1) s when k1 >= s (the conv1 ring holds k1 - s rows)
        if e >= T:
            ref = b.om.predict_with_logits(frames[None, e - T:e])[1][0]
            assert abs(z[n] - ref) <= 1e-9, (cid, n, z[n], ref)
            checked += 1
    assert checked >= 20, (cid, checked)


def test_warm_anchor_covers_the_four_kinds():
    kinds = set()
    for cid in STREAM_IDS:
        d = vc.case(cid).desc
        if d["t_final"] > 1:
            kinds.add((bool(any(d["residual"])), d["pool"]))
    assert {(True, 0), (True, "average"), (True, "max")} <= kinds   # pooling without a residual: the test below


def test_pooled_only_warm_anchor():
    """pooled average and pooled max without any residual (the case list always pairs pooling with a residual block)"""
    for pool in ("average", "max"):
        d = vc.desc_of(5, 3, 2, [(1, (3, 5), 6)], 4, pool=pool)
        flags, T = vc.flags_of(d), d["frames"]
        om = ec.perturbed_oracle(T, seed=5, flags=flags)
        net = vo.Net(flags, om, T)
        frames = np.random.default_rng(3).uniform(0, 26, size=(T + 40, 40))
        z = vo.whole_sequence(net, frames)
        zs = vo.StepStream(net).run(frames)
        assert np.abs(z - zs).max() <= 1e-9
        for n in range(z.size):
            e = (n + 1) * 2
            if e >= T:
                assert abs(z[n] - om.predict_with_logits(frames[None, e - T:e])[1][0]) <= 1e-9


def test_description_derives_t_final_from_the_flags():
    flags = dict(ec.DEF, pooled=1, residual_connection="1,0,1,0")
    lay = GraphMixedNetLayout(flags, 52)
    assert lay.t_last == 1
    d = streaming.mixednet_stream_description(flags, 52, 1, "stream")
    assert d["t_final"] == vo.t_final_of(flags, 52) > 1 and d["pool"] == "average" and d["residual"] == [1, 0, 1, 0] and d["attention"] == 0
    assert streaming.mixednet_stream_description(dict(flags, max_pool=1), 52, 1, "non_stream")["pool"] == "max"
    # the hole this closes: the old description of the same pooled model says t_final 1 and does not raise
    assert streaming.stream_description(dict(ec.DEF, pooled=1), lay.t_last, 52, 1, "stream")["t_final"] == 1
    # T_f = 1: the head flags do nothing and are dropped
    d1 = vc.desc_of(5, 3, 1, [(1, (3,), 7)], 1)
    got = streaming.mixednet_stream_description(dict(vc.flags_of(d1), pooled=1, spatial_attention=1), d1["frames"], 1, "stream")
    assert (got["t_final"], got["pool"], got["attention"]) == (1, 0, 0)
    # attention: non_stream only, at least 4 frames
    att = dict(ec.DEF, spatial_attention=1)
    assert streaming.mixednet_stream_description(att, 52, 1, "non_stream")["attention"] == 1
    with pytest.raises(NotImplementedError, match="spatial_attention in stream mode.*CURRENT attention value"):
        streaming.mixednet_stream_description(att, 52, 1, "stream")
    d3 = vc.desc_of(5, 3, 1, [(1, (3,), 7)], 3)
    with pytest.raises(ValueError, match="at least 4 frames"):
        streaming.mixednet_stream_description(dict(vc.flags_of(d3), spatial_attention=1), d3["frames"], 1, "non_stream")
    with pytest.raises(NotImplementedError, match="first_conv_filters = 0"):
        streaming.mixednet_stream_description(dict(flags, first_conv_filters=0), 52, 1, "stream")
    with pytest.raises(ValueError, match="stride"):
        streaming.mixednet_stream_description(flags, 52, 2, "stream")
    # every case's description is what the function derives from the case's flags
    for c in vc.cases():
        mode = "non_stream" if c.desc["attention"] else "stream"
        got = streaming.mixednet_stream_description(vc.flags_of(c.desc), c.desc["frames"], c.desc["stride"], mode)
        want = dict(c.desc, mode=mode, pool=c.desc["pool"] if c.desc["t_final"] > 1 else 0)
        assert got == want, (c.id, got, want)


def test_old_description_is_unchanged():
    d = streaming.stream_description(ec.DEF, 5, 52, 1, "stream")
    assert sorted(d) == ["blocks", "conv1_filters", "conv1_kernel", "frames", "mode", "stride", "t_final"]
    for bad, name in ((dict(residual_connection="1,0,0,0"), "residual_connection"), (dict(spatial_attention=1), "spatial_attention"),
                      (dict(pooled=1), "pooled"), (dict(first_conv_filters=0), "first_conv_filters")):
        with pytest.raises(NotImplementedError, match=name):
            streaming.stream_description(dict(ec.DEF, **bad), 5, 52, 1, "stream")


class _NoDevice:
    """a model whose device side must not be touched"""

    def __init__(self, flags):
        self.flags = flags
        self.layout = GraphMixedNetLayout(flags, 52)

    def __getattr__(self, name):
        raise AssertionError("the refusal must come before the model's %s is used" % name)


@pytest.mark.parametrize("bad,name", [(dict(residual_connection="1,0,1,0"), "residual_connection"), (dict(pooled=1), "pooled"),
                                      (dict(spatial_attention=1), "spatial_attention")])
def test_quantize_refuses_before_any_device_work(bad, name):
    model = _NoDevice(dict(ec.DEF, **bad))
    with pytest.raises(NotImplementedError, match=name):
        quantize.calibrate(model, None, {"stride": 1, "spectrogram_length": 52})
    with pytest.raises(NotImplementedError, match=name):
        quantize.quantize(model, np.zeros((4, 2), np.float32))


def _config_file(tmp_path):
    import yaml
    cfg = {"train_dir": str(tmp_path / "run"), "clip_duration_ms": 1500, "batch_size": 8, "features": []}
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.dump(cfg))
    return str(path), tmp_path / "run"


@pytest.mark.parametrize("argv,name", [
    (["--test_tflite_streaming", "1", "mixednet", "--residual_connection", "0,0,0,0", "--spatial_attention", "1"],
     "spatial_attention in stream mode"),
    (["--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "mixednet", "--residual_connection", "1,0,1,0"], "residual_connection"),
    (["--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "mixednet", "--residual_connection", "0,0,0,0",
      "--first_conv_filters", "0"], "first_conv_filters = 0"),
    (["--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "mixednet", "--residual_connection", "0,0,0,0",
      "--pooled", "1"], "pooled"),
    (["--test_tflite_streaming_quantized", "1", "--quantized_backend", "native", "mixednet", "--residual_connection", "0,0,0,0",
      "--spatial_attention", "1"], "spatial_attention"),
])
def test_cli_refuses_before_training(tmp_path, monkeypatch, argv, name):
    """--train 1: the refusal arrives before a model is built, before training and before train_dir is claimed"""
    path, run = _config_file(tmp_path)

    def no_model(*a, **k):
        raise AssertionError("the topology check must run before the model is built")
    monkeypatch.setattr(model_train_eval.mixednet, "model", no_model)
    with pytest.raises(NotImplementedError, match=name):
        model_train_eval.main(["--training_config", path, "--train", "1"] + argv)
    assert not run.exists()


def test_cli_lets_the_covered_evaluations_through_the_early_check(tmp_path):
    path, _ = _config_file(tmp_path)
    for extra in (["--residual_connection", "1,0,1,0", "--pooled", "1"], ["--residual_connection", "0,0,0,0", "--pooled", "1", "--max_pool", "1"]):
        flags = model_train_eval.build_parser().parse_args(
            ["--training_config", path, "--test_tf_nonstreaming", "1", "--test_tflite_nonstreaming", "1", "--test_tflite_streaming", "1",
             "mixednet"] + extra)
        model_train_eval.check_evaluation_flags(flags, model_train_eval.mixednet, model_train_eval.load_config(flags, model_train_eval.mixednet))
    flags = model_train_eval.build_parser().parse_args(
        ["--training_config", path, "--test_tf_nonstreaming", "1", "--test_tflite_nonstreaming", "1", "mixednet",
         "--residual_connection", "0,0,0,0", "--spatial_attention", "1"])
    model_train_eval.check_evaluation_flags(flags, model_train_eval.mixednet, model_train_eval.load_config(flags, model_train_eval.mixednet))


def test_stream_refuses_an_unknown_pool_name():
    from microwakeword_amd import native

    class _Engine:
        nl = None
    with pytest.raises(ValueError, match="'average' or 'max'"):
        native.Stream(_Engine(), dict(vc.desc_of(4, 3, 1, [(1, (3,), 4)], 2), pool="avg"))
