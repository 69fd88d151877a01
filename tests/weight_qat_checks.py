"""Checks of weight-only quantization-aware training (the engine's ``weight_qat`` option, csrc/kernels_qat.hip.h, and
``microwakeword_amd/qat.py``), shared by tests/test_weight_qat_emulated.py (tests/hipemu) and tests/test_weight_qat_gpu.py,
the same shapes on both.

Three small models cover the three layouts: (a) a MixedNet on the specialised block kernels, (b) a residual / pooled MixedNet
on the conv/BN graph engine, (c) an Inception model.  The shadow is compared byte for byte with ``qat.fake_quant_weights``
(which calls ``quantize.weight_params``).  A train step is held to the float64 oracle's step AT THE SHADOW with the bounds
engine_checks applies to the float step: the existing checks run unchanged, against an oracle whose forward reads the
fake-quantized weights while its Adam keeps the master (``QatOracle``) and an engine that has the option on (``QatEngine``).
"""
import contextlib

import numpy as np
import pytest
import torch

import engine_checks as ec
from microwakeword_amd import native, qat
from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout, MixedNetLayout
from oracle import model_oracle as mo

B, T = 8, 60
# (a) two blocks, widths 32 and 48, a one-kernel MixConv and a two-group MixConv (fused table with masked taps), conv1 32 x 3
BLOCK = dict(ec.DEF, pointwise_filters="32,48", residual_connection="0,0", repeat_in_block="1,1", mixconv_kernel_sizes="[5],[7,11]",
             first_conv_filters=32, first_conv_kernel_size=3)
# (b) the graph family: a residual block with two repeats, a width that is no multiple of 32, pooled head: the dense kernel has 24
# elements (fewer than a wave); its longest channel is conv1's 6 x 40 = 240 (the graph engine takes kernel x channels <= 256, and
# a pooled head leaves no longer one: the channels longer than a workgroup's threads are in (a) and (c))
GRAPH = dict(mo.MIXEDNET_DEFAULTS, residual_connection="1,0", pointwise_filters="24,24", repeat_in_block="2,1",
             mixconv_kernel_sizes="[5],[3,7]", first_conv_filters=16, first_conv_kernel_size=6, stride=1, pooled=1)
# (c) one stem and one block at reduced filter counts
INCEPTION = dict(cnn1_filters="16", cnn1_kernel_sizes="5", cnn1_subspectral_groups="4", cnn2_filters1="12", cnn2_filters2="16",
                 cnn2_kernel_sizes="3", cnn2_subspectral_groups="1", cnn2_dilation="1", dropout=0.2)
KINDS = ("block", "graph", "inception")


def layout_of(kind, frames=T):
    if kind == "block":
        return MixedNetLayout(BLOCK, frames)
    if kind == "graph":
        return GraphMixedNetLayout(GRAPH, frames)
    return InceptionLayout(INCEPTION, frames)


def flags_of(kind):
    return {"block": BLOCK, "graph": GRAPH, "inception": INCEPTION}[kind]


def new_engine(lib, kind, max_batch=B, cls=native.Engine):
    lay = layout_of(kind)
    eng = cls(lib=lib, **lay.engine_args(max_batch))
    if kind != "inception":
        eng.set_grad_mask(lay.grad_mask())
    return lay, eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_shadow(eng, lay, what=""):
    """check 1 on the engine's current master: the vector the next forward reads is the restatement, bit for bit"""
    master = eng.get_params()
    got = eng.get_forward_params()
    want = qat.forward_params_reference(lay, master)
    if not same_bits(got, want):
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        raise AssertionError("%s: shadow differs from the restatement at %d of %d parameters, first %d: %r vs %r (master %r)"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], master[bad[0]]))
    outside = np.ones(master.size, bool)
    outside[qat.channel_map(lay)[1]] = False
    assert same_bits(got[outside], master[outside]), what   # biases, gamma / beta, masked taps: the master's bits
    return got, master


# ------------------------------------------------------------------------------------------------- 1. the shadow, bit for bit
def random_weights(lay, seed):
    rng = np.random.default_rng(seed)
    ws = []
    for name, shape, _ in lay.keras_vars:
        if name.endswith("moving_variance"):
            ws.append((1.0 + np.abs(rng.normal(0, 0.2, shape))).astype(np.float32))
        else:
            ws.append(rng.normal(0, 0.3, shape).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 2)))
    return ws


def crafted_weights(lay):
    """random weights with, in the first convolution kernel: an all-zero channel, a channel whose extreme is negative, a channel
    with amax 127 and the ties 0.5, 1.5, -2.5, 126.5 (half-away: 1, 2, -3, 127; half-even would differ) and entries at +-amax,
    a channel with a denormal entry; the dense kernel is the one-channel kernel"""
    ws = random_weights(lay, 5)
    vi = next(i for i, (n, s, _) in enumerate(lay.keras_vars) if len(s) == 4 and qat.kernel_axis(n, s) == 3 and s[3] >= 4 and s[0] * s[2] >= 8)
    k = ws[vi]
    flat = k.reshape(-1, k.shape[3])   # a view: [k * cin, cout]
    flat[:, 0] = 0.0
    flat[:, 1] = np.abs(flat[:, 1])
    flat[3, 1] = -3.0 * flat[:, 1].max()
    flat[:, 2] = 0.0
    flat[:6, 2] = [127.0, 0.5, 1.5, -2.5, 126.5, -127.0]
    flat[2, 3] = np.float32(1e-40)
    assert flat[2, 3] != 0 and abs(flat[2, 3]) < np.finfo(np.float32).tiny
    return ws, vi


def check_shadow_bits(lib, kind):
    lay, eng = new_engine(lib, kind)
    start, elem = qat.channel_map(lay)
    sizes = np.diff(start)
    assert sizes.max() > (64 if kind == "graph" else 256) and sizes.min() < 64, (sizes.max(), sizes.min())   # more than a workgroup's threads / fewer than a wave
    assert 1 in [s[1] for n, s, _ in lay.keras_vars if n == "dense.kernel"]
    eng.set_weight_qat_map(start, elem)
    eng.set_option("weight_qat", 1)
    rng = np.random.default_rng(3)
    eng.set_batch(ec.synth_x(rng, B, T))
    ws, vi = crafted_weights(lay)
    p, s = lay.pack(ws)
    eng.set_params(p)
    eng.set_bn_state(s)
    eng.forward(B, training=False)
    got, master = assert_shadow(eng, lay, kind + " crafted")
    assert same_bits(master, p)   # the master is untouched
    # the crafted channels by hand
    sh = lay.unpack(got, s)[vi].reshape(-1, ws[vi].shape[3])
    assert not sh[:, 0].any() and sh[3, 1] < 0 and -sh[3, 1] == np.abs(sh[:, 1]).max() and sh[:, 1].max() < -sh[3, 1]   # q = -127, nothing at +127
    assert sh[:6, 2].tolist() == [127.0, 1.0, 2.0, -3.0, 127.0, -127.0] and sh[2, 3] == 0.0
    assert np.abs(got[elem] - master[elem]).max() > 0   # it is a grid
    # masked MixConv taps set to nonzero in the native vector: outside every channel, copied through, no channel's scale moves
    masked = np.nonzero(lay.grad_mask() == 0)[0] if kind != "inception" else np.zeros(0, np.int64)
    if kind != "inception":
        assert masked.size and not np.isin(masked, elem).any()
        p2 = p.copy()
        p2[masked] = 1000.0
        eng.set_params(p2)
        eng.forward(B, training=False)
        got2, _ = assert_shadow(eng, lay, kind + " masked taps")
        assert np.all(got2[masked] == 1000.0) and same_bits(got2[elem], got[elem])
    # a channel whose maximum is not finite is copied through; the others are not disturbed
    p3 = p.copy()
    first, second = elem[start[1]:start[2]], elem[start[2]:start[3]]
    p3[first[0]], p3[second[1]] = np.inf, np.nan
    eng.set_params(p3)
    eng.forward(B, training=False)
    got3 = eng.get_forward_params()
    assert same_bits(got3[first], p3[first]) and same_bits(got3[second], p3[second])
    rest = np.setdiff1d(elem, np.concatenate([first, second]))
    assert same_bits(got3[rest], got[rest])
    assert same_bits(got3, qat.forward_params_reference(lay, p3))
    for seed in (11, 12, 13):
        p, s = lay.pack(random_weights(lay, seed))
        eng.set_params(p)
        eng.forward(B, training=False)
        assert_shadow(eng, lay, "%s seed %d" % (kind, seed))
    eng.close()


# ------------------------------------------------------------------------------- 3 / 6. a train step is the oracle's step at the shadow
class QatOracle(mo.OracleModel):
    """The float64 oracle whose forward and backward read ``fake_quant_weights(master)`` while ``train_step``'s KerasAdam keeps
    updating the master (``get_weights``): the gradient it applies is the one taken at the shadow."""

    def __init__(self, base, lay, state):
        super().__init__(base.kind, base.flags, base.T, dtype=base.dtype)
        self.set_weights(base.get_weights())
        self.lay, self.state = lay, state
        assert [tuple(v.value.shape) for v in self.vars] == [s for _, s, _ in lay.keras_vars]

    def _tensors(self, requires_grad):
        if not self.state["on"]:
            return super()._tensors(requires_grad)
        t = {}
        for v, w in zip(self.vars, qat.fake_quant_weights(self.lay, [v.value for v in self.vars])):
            x = torch.tensor(w, dtype=self.dtype)
            if requires_grad and v.trainable:
                x.requires_grad_(True)
            t[v.name] = x
        return t


@contextlib.contextmanager
def qat_run(monkeypatch, lay, on_from_step=0):
    """inside: engines that engine_checks creates have the option on from their train step number ``on_from_step`` (0-based) and
    check 1 after every step and every set_params; the oracles it creates are QatOracles switched on at the same step"""
    state = dict(on=on_from_step == 0, steps=0, checked=0)
    cmap = qat.channel_map(lay)

    class QatEngine(native.Engine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.set_weight_qat_map(*cmap)
            if state["on"]:
                self.set_option("weight_qat", 1)

        def train_step(self, *a, **k):
            if state["steps"] == on_from_step and not state["on"]:
                self.set_option("weight_qat", 1)
                state["on"] = True
            super().train_step(*a, **k)
            state["steps"] += 1
            if state["on"]:
                assert_shadow(self, lay, "after step %d" % state["steps"])
                state["checked"] += 1

        def set_params(self, a):
            super().set_params(a)
            if state["on"]:   # seen by the next forward
                assert_shadow(self, lay, "after set_params")

    def wrap(make):
        return lambda *a, **k: QatOracle(make(*a, **k), lay, state)
    with monkeypatch.context() as m:
        m.setattr(native, "Engine", QatEngine)
        m.setattr(ec, "perturbed_oracle", wrap(ec.perturbed_oracle))
        m.setattr(ec, "perturbed_inception_oracle", wrap(ec.perturbed_inception_oracle))
        yield state


def run_family_check(lib, kind, steps, graphs=False):
    """engine_checks' train-step check of the family, unchanged: its bounds, its imposed ReLU masks, its metric comparison"""
    if kind == "block":
        return ec.check_train_steps(lib, B=B, T=T, steps=steps, grid=2, flags=BLOCK, graphs=graphs)
    if kind == "graph":
        return ec.check_graph_mixednet(lib, flags=GRAPH, B=B, T=T, steps=steps, grid=2, graphs=graphs)
    return ec.check_inception_train_steps(lib, B=B, T=T, steps=steps, grid=2, flags=INCEPTION, graphs=graphs)


def check_train_steps_at_the_shadow(lib, kind, monkeypatch, steps=3):
    lay = layout_of(kind)
    with qat_run(monkeypatch, lay) as state:
        run_family_check(lib, kind, steps)
    assert state["on"] and state["steps"] == steps and state["checked"] == steps
    # the comparison has teeth: the float oracle's step is outside the bounds (the shadow is not the master)
    with pytest.raises(AssertionError):
        with monkeypatch.context() as m:
            cmap = qat.channel_map(lay)

            class OnEngine(native.Engine):
                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    self.set_weight_qat_map(*cmap)
                    self.set_option("weight_qat", 1)
            m.setattr(native, "Engine", OnEngine)
            run_family_check(lib, kind, 1)


def check_toggle_mid_run(lib, kind, monkeypatch):
    """2 float steps, the option on, 2 steps: every step is the oracle's (float, then at the shadow)"""
    with qat_run(monkeypatch, layout_of(kind), on_from_step=2) as state:
        run_family_check(lib, kind, 4)
    assert state["on"] and state["steps"] == 4 and state["checked"] == 2


# ------------------------------------------------------------------------------------------------- 4. inference
def check_inference(lib, kind):
    lay, eng = new_engine(lib, kind)
    flags = flags_of(kind)
    base = ec.perturbed_inception_oracle(T, flags) if kind == "inception" else ec.perturbed_oracle(T, flags=flags)
    om = QatOracle(base, lay, dict(on=True))
    p, s = lay.pack(om.get_weights())
    eng.set_params(p)
    eng.set_bn_state(s)
    eng.set_weight_qat_map(*qat.channel_map(lay))
    eng.set_option("weight_qat", 1)
    rng = np.random.default_rng(7)
    x = ec.synth_x(rng, B, T)
    want = torch.sigmoid(om.logits(x, False)[0]).detach().numpy().reshape(-1)
    plain = torch.sigmoid(base.logits(x, False)[0]).detach().numpy().reshape(-1)
    eng.set_batch(x)
    eng.forward(B, training=False)
    got = eng.read_outputs(B, want_loss=False)[0]
    assert np.abs(got - want).max() <= ec.FWD_TOL, np.abs(got - want).max()
    # window evaluation, in one batch and in batches of 3 (the shadow of the first batch serves the others)
    eng.upload_store(0, x.reshape(-1))
    win = np.array([(0, 0, T, 0, i * T * 40) for i in range(B)], native.WINDOW_DTYPE)
    y = (rng.random(B) < 0.5).astype(np.float32)
    for batch in (B, 3):
        eng.metrics_reset()
        eng.evaluate_windows(win, y, batch)
        n_last = B - (B - 1) // batch * batch
        tail = eng.read_outputs(n_last, want_loss=False)[0]
        assert np.abs(tail - want[B - n_last:]).max() <= ec.FWD_TOL, (batch, np.abs(tail - want[B - n_last:]).max())
        m = native.metrics_from_raw(eng.metrics_raw())
        assert m["tp"][0] + m["fn"][0] == int(y.sum()) and m["tp"][0] + m["fp"][0] + m["tn"][0] + m["fn"][0] == B
    # off again: the master's inference
    eng.set_option("weight_qat", 0)
    eng.set_batch(x)
    eng.forward(B, training=False)
    off = eng.read_outputs(B, want_loss=False)[0]
    assert np.abs(off - plain).max() <= ec.FWD_TOL
    eng.close()
    return float(np.abs(want - plain).max())


# ------------------------------------------------------------------------------------------------- 5 / 7 / 8. off, replay, refusals
def three_steps(lib, kind, prepare=None, steps=3, seed=21):
    """`steps` train steps on fixed batches from fixed weights -> (params, BN state, Adam m, v, step, gradient) and the engine"""
    lay, eng = new_engine(lib, kind)
    p, s = lay.pack(random_weights(lay, 4))
    s = np.abs(s) + np.float32(0.5)
    p = p * (lay.grad_mask() if kind != "inception" else 1.0)
    eng.set_params(p.astype(np.float32))
    eng.set_bn_state(s)
    if kind == "inception":
        eng.set_option("dropout_seed", 9)
    if prepare is not None:
        prepare(eng, lay)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        eng.set_batch(ec.synth_x(rng, B, T))
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), rng.choice([0.5, 1.0, 2.0], size=B).astype(np.float32))
        eng.train_step(B, 1e-2)
    m, v, step = eng.get_opt_state()
    return (eng.get_params(), eng.get_bn_state(), m, v, np.int64(step), eng.get_grads()), eng, lay


def all_same(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def check_off_is_off(lib, kind):
    plain, eng_a, lay = three_steps(lib, kind)
    assert all(np.all(np.isfinite(a)) for a in plain)

    def on_then_off(eng, lay):
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)
        eng.set_option("weight_qat", 0)
    toggled, eng_b, _ = three_steps(lib, kind, on_then_off)
    assert all_same(plain, toggled)
    for eng in (eng_a, eng_b):   # with the option off the forward reads the master
        assert same_bits(eng.get_forward_params(), eng.get_params())

    def on(eng, lay):
        eng.set_weight_qat_map(*qat.channel_map(lay))
        eng.set_option("weight_qat", 1)
    trained, eng_c, _ = three_steps(lib, kind, on)
    assert not same_bits(trained[0], plain[0])   # ... and on is not off
    eng_c.set_weight_qat_map(np.zeros(0, np.int32), np.zeros(0, np.int32))   # no channels: the map is gone, the option off
    assert same_bits(eng_c.get_forward_params(), eng_c.get_params())
    with pytest.raises(native.NativeError, match="error -1: .*channel map"):
        eng_c.set_option("weight_qat", 1)
    for eng in (eng_a, eng_b, eng_c):
        eng.close()


def check_graph_replay(lib):
    """graphs = 1 with the option on: the refresh is one more node of the captured chain - 3 steps equal the eager run's"""
    def on(graphs):
        def prepare(eng, lay):
            eng.set_weight_qat_map(*qat.channel_map(lay))
            eng.set_option("weight_qat", 1)
            eng.set_option("graphs", graphs)
        return prepare
    eager, eng_a, lay = three_steps(lib, "block", on(0))
    replay, eng_b, _ = three_steps(lib, "block", on(1))
    assert all_same(eager, replay)
    assert_shadow(eng_b, lay, "after replay")
    plain, eng_c, _ = three_steps(lib, "block")
    assert not same_bits(plain[0], replay[0])
    for eng in (eng_a, eng_b, eng_c):
        eng.close()


def check_refusals(lib, kind):
    fresh, eng_f, lay = three_steps(lib, kind, steps=1)
    eng_f.close()
    start, elem = qat.channel_map(lay)

    def refused(eng, lay):
        P = eng.n_params

        def no(call, word):
            with pytest.raises(native.NativeError, match="error -1: .*" + word):
                call()
        no(lambda: eng.set_option("weight_qat", 1), "channel map")
        bad = elem.copy()
        bad[5] = P
        no(lambda: eng.set_weight_qat_map(start, bad), "outside the parameter vector")
        bad[5] = -1
        no(lambda: eng.set_weight_qat_map(start, bad), "outside the parameter vector")
        bad = elem.copy()
        bad[7] = bad[2]
        no(lambda: eng.set_weight_qat_map(start, bad), "two channels")
        down = start.copy()
        down[2], down[3] = start[3], start[2]
        no(lambda: eng.set_weight_qat_map(down, elem), "ascending")
        no(lambda: eng.set_weight_qat_map(start[:-1], elem), "from 0 to n_elems")
        no(lambda: eng.set_option("weight_qat", 1), "channel map")   # none of them left a map behind
        no(lambda: eng.set_option("weight_qat", 2), "0 or 1")
        assert same_bits(eng.get_forward_params(), eng.get_params())
    after, eng, _ = three_steps(lib, kind, refused, steps=1)
    assert all_same(fresh, after)   # the context is usable: the float step of a fresh context
    # a refused map leaves an installed one in place
    eng.set_weight_qat_map(start, elem)
    eng.set_option("weight_qat", 1)
    with pytest.raises(native.NativeError, match="two channels"):
        eng.set_weight_qat_map(start, np.where(np.arange(elem.size) == 7, elem[2], elem))
    assert_shadow(eng, lay, "after a refused replacement")
    eng.close()


# ------------------------------------------------------------------------------------------------- 9. the loop
def loop_config(tmp_path, name, first_step=5, **over):
    import int8_in_loop_checks as ilc
    import streaming_validation_checks as svc
    cfg = svc.config(tmp_path, name, ilc.SVQ, prefetch_batches=0, **over)
    if first_step is not None:
        cfg["weight_quantization_aware"] = dict(first_step=first_step)
    return cfg


def kernels_off_grid(model, weights):
    """how many kernel entries of a Keras weight list differ from their fake-quantized value"""
    fq = qat.fake_quant_weights(model, weights)
    return sum(int((a != b).sum()) for a, b in zip(weights, fq))


def check_loop(lib, tmp_path, caplog):
    import logging
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    cfg = loop_config(tmp_path, "qat")
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        model, _ = smc.run_loop(lib, cfg)
    said = [r.getMessage() for r in caplog.records if "weight quantization-aware" in r.getMessage()]
    assert len(said) == 1 and said[0].startswith("Step #5:"), said   # on before step 5's forward: steps 1..4 are float
    lines = svc.log_of(cfg, "train")
    assert [(e["step"], e["weight_qat"]) for e in lines] == [(4, 0), (8, 1), (12, 1)]
    assert model.weight_qat and any("fake-quantized" in line for line in summary_of(model))
    # what is saved is the fp32 master, not the grid
    best = svc.file_arrays(cfg["train_dir"] + "/best_weights.weights.h5")
    arrays = [np.frombuffer(best[k], np.float32).reshape(s) for k, (_, s, _) in zip(sorted(best), model.layout.keras_vars)]
    assert kernels_off_grid(model, arrays) > 0
    final = model.get_weights()
    assert kernels_off_grid(model, final) > 0 and kernels_off_grid(model, model.get_forward_weights()) == 0
    assert [e["step"] for e in svc.log_of(cfg, "validation_streaming")] == [0] + svc.BOUNDARIES
    # stopped after step 8 and restored: the same final weights as the uninterrupted run
    cut = loop_config(tmp_path, "cut", training_steps=[6, 2])
    smc.run_loop(lib, cut)
    rest = dict(cut, training_steps=[4], learning_rates=[cfg["learning_rates"][1]])
    import mining_checks as mc
    state = mc.rng_state()
    from microwakeword_amd import mixednet
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    import random
    random.seed(1)   # the handler orders its sample lists on the global generators when it is made: as run_loop makes it ...
    np.random.seed(1)
    restored = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=99, max_batch=64)
    fh = FeatureHandler(rest, engine=restored.engine)
    random.setstate(state[0])   # ... and the draws go on where the stopped run left them
    np.random.set_state(state[1])
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        tr.train(restored, rest, fh, verbose=False)
    said = [r.getMessage() for r in caplog.records if "weight quantization-aware" in r.getMessage()]
    assert len(said) == 1 and said[0].startswith("Step #9:"), said   # re-derived from the restored optimizer step
    assert restored.engine.get_opt_state()[2] == 12
    assert [w.tobytes() for w in restored.get_weights()] == [w.tobytes() for w in final]
    return cfg


def summary_of(model):
    lines = []
    model.summary(print_fn=lines.append)
    return lines


def check_loop_without_the_key(lib, tmp_path):
    """no key: the weights of a run in which the option never existed; the train scalars carry no weight_qat field"""
    import stream_mine_checks as smc
    import streaming_validation_checks as svc
    cfg = loop_config(tmp_path, "plain", first_step=None)
    model, _ = smc.run_loop(lib, cfg)
    assert not getattr(model, "weight_qat", False) and all("weight_qat" not in e for e in svc.log_of(cfg, "train"))
    assert not any("fake-quantized" in line for line in summary_of(model))
    # the same run with first_step beyond its last step: the map is never installed, the option never set
    late = loop_config(tmp_path, "late", first_step=13)
    model_l, _ = smc.run_loop(lib, late)
    assert [w.tobytes() for w in model.get_weights()] == [w.tobytes() for w in model_l.get_weights()]
    assert [e["weight_qat"] for e in svc.log_of(late, "train")] == [0, 0, 0]


def check_loop_refusals(lib, tmp_path):
    """unknown key, negative or non-integer first_step: a ValueError that names the key, before the first step and before any
    file exists under train_dir"""
    import os
    import yaml
    import stream_mine_checks as smc
    from microwakeword_amd import mixednet, model_train_eval
    from microwakeword_amd import train as tr
    from microwakeword_amd.data import FeatureHandler
    cases = ((dict(first_step=-1), "first_step"), (dict(first_step=2.5), "first_step"), (dict(first_step="5"), "first_step"),
             (dict(first_step=True), "first_step"), (dict(first_step=3, last_step=9), "last_step"), ([5], "mapping"))
    model = mixednet.model(ec.DEF, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)
    for n, (bad, word) in enumerate(cases):
        cfg = loop_config(tmp_path, "bad%d" % n, first_step=None)
        cfg["weight_quantization_aware"] = bad
        with pytest.raises(ValueError, match="weight_quantization_aware.*" + word):
            tr.train(model, cfg, FeatureHandler(cfg, engine=model.engine), verbose=False)
        assert model.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=smc.B_LOOP, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet", "--residual_connection", "0,0,0,0"]
    for bad, word in cases:
        with open(tmp_path / "training_parameters.yaml", "w") as out:
            yaml.safe_dump(dict(base, weight_quantization_aware=bad), out)
        with pytest.raises(ValueError, match="weight_quantization_aware.*" + word):
            model_train_eval.main(argv)
        assert not train_dir.exists()
