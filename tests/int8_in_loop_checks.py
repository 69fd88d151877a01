"""Checks of the int8 model inside the training loop, shared by the emulator tests (tests/test_int8_in_loop_emulated.py) and the
GPU tests (tests/test_int8_in_loop_gpu.py), the same shapes on both:

  * ``mww_stream_calibrate`` (csrc/tu_stream_calibrate.hip): ranges against ``mww_stream_calibrate_host`` on the host rows of the
    same windows, outputs and rings against ``mww_stream_run``;
  * ``quantize.calibration_windows``: the fixed calibration set and the generators it leaves alone;
  * the ``quantized`` key of ``streaming_validation`` / ``hard_negative_mining`` in the 12-step loop of
    tests/stream_mine_checks.py, against a restatement through ``calibrate_host`` on host rows.

Every comparison is exact."""
import os
import random

import numpy as np
import pytest

from microwakeword_amd import mining, native, quantize, quantize_graph, quantize_mixednet, streaming
from microwakeword_amd import train as tr
from microwakeword_amd.data import FeatureHandler
import engine_checks as ec
import mining_checks as mc
import quant_mixednet_checks as qmc
import stream_mine_checks as smc
import stream_sweep as ss
import streaming_checks as sc
import streaming_validation_checks as svc

T_WIN = 60   # the windows of the kernel cases: T_WIN rows cut to T_WIN - stride, as calibration_windows cuts them
TILE = ss.TILE


# ------------------------------------------------------------------------------------------------- mww_stream_calibrate
class KernelCase:
    """one int8-capable stream description with float weights in the shared context: ``new()`` a fresh stream holding the
    weights, ``refused()`` the same description on the creator without the int8 entry points (None: a plain MixedNet has
    none), ``quantized(ranges)`` its int8 model"""

    def __init__(self, lib, name):
        self.engine = sc.context_model(lib).engine
        self.model = sc.context_model(lib)
        if name in ("plain-s1", "plain-s3"):
            s = 1 if name == "plain-s1" else 3
            self.desc = ss.desc_of(5, 4, s, [(1, (3,), 8), (1, (3, 5), 6)], 3)
            weights = ec.perturbed_oracle(self.desc["frames"], flags=sc.flags_of(self.desc)).get_weights()
            self.new_raw = lambda: native.Stream(self.engine, self.desc)
            self.refused = None
            self.quantized = lambda r: quantize.quantize_weights(self.desc, weights, r)
        elif name == "residual-pooled":
            b = qmc.built("tile-edges_grid_avg-tf5_res")
            self.desc, weights = b.desc, b.weights
            assert any(self.desc["residual"]) and self.desc["pool"]
            self.new_raw = lambda: native.Stream(self.engine, self.desc, int8=True)
            self.refused = lambda: native.Stream(self.engine, self.desc)
            self.quantized = lambda r: quantize_mixednet.quantize_weights(self.desc, weights, r)
        else:
            assert name == "inception"
            self.desc = streaming.graph_stream_description(ec.INC, T_WIN, 1, "stream")
            weights = ec.perturbed_inception_oracle(T_WIN, ec.INC).get_weights()
            self.new_raw = lambda: native.GraphStream(self.engine, self.desc, int8=True)
            self.refused = lambda: native.GraphStream(self.engine, self.desc)
            self.quantized = lambda r: quantize_graph.quantize_weights(self.desc, weights, r)
        self.stride = int(self.desc["stride"])
        self.flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in weights])

    def new(self, raw=None):
        st = (raw or self.new_raw)()
        st.set_weights(self.flat)
        return st

    def tracks(self):
        """windows of T_WIN - stride rows, even ones in a u16 store and odd ones in an f32 store, some padded in front (one
        of them all padding), enough for two 256-output tiles: 8 at stride 1, 16 at stride 3"""
        rows, n = T_WIN - self.stride, 8 if self.stride == 1 else 16
        pads = [0] * n
        pads[1], pads[2], pads[5] = 7, 1, rows
        return sc.Tracks(self.model, [rows] * n, pads, seed=3)


KERNEL_CASES = ("plain-s1", "plain-s3", "residual-pooled", "inception")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_calibrate(lib, name):
    c = KernelCase(lib, name)
    tr_ = c.tracks()
    rows = np.concatenate(tr_.frames)
    assert rows.shape[0] % c.stride == 0 and rows.shape[0] // c.stride > TILE   # two tiles, two workgroups
    # the host form on a fresh stream, on the host rows of the same windows
    h = c.new()
    want = h.calibrate_host(rows)
    p_h, z_h = h.read(want_logits=True)
    # the float run of the same tracks
    r = c.new()
    off_r = r.run(tr_.win)
    p_r, z_r = r.read(want_logits=True)
    st_r = r.get_state()
    assert same_bits(p_r, p_h) and same_bits(z_r, z_h)   # (the concatenated stream IS the track run: every track whole strides)
    a = c.new()
    off, ranges = a.calibrate(tr_.win)
    assert ranges.dtype == np.float32 and ranges.shape == (a.num_tensors(), 2)
    assert np.array_equal(ranges, want), (name, ranges, want)
    assert np.all(np.isfinite(ranges)) and ranges[0, 0] == 0.0 and ranges[0, 1] == rows.max() and ranges[0, 1] > 40.0   # pad zeros; the u16 scale
    assert np.array_equal(off, off_r) and off[-1] == rows.shape[0] // c.stride == a.n_out
    p, z = a.read(want_logits=True)
    assert same_bits(p, p_r) and same_bits(z, z_r)
    assert same_bits(a.get_state(), st_r) and same_bits(a.get_state(), h.get_state())
    # the state is carried on: a second call continues the stream
    few = tr_.win[3:6]
    off2, ranges2 = a.calibrate(few)
    want2 = h.calibrate_host(np.concatenate(tr_.frames[3:6]))
    assert np.array_equal(off2, r.run(few)) and np.array_equal(ranges2, want2)
    assert same_bits(a.read(), r.read()) and same_bits(a.get_state(), r.get_state())
    # with int8 parameters loaded and an int8 run behind it: the call on a fresh stream
    q = c.new()
    q.set_quantized(*c.quantized(quantize.widen_input_range(ranges)).packed())
    q.run(tr_.win)
    u8 = q.read_q8()
    assert not same_bits(q.read(), p_r)   # that was the int8 kernel
    off_q, ranges_q = q.calibrate(tr_.win)
    assert np.array_equal(ranges_q, ranges) and np.array_equal(off_q, off)
    assert same_bits(q.read(), p_r) and same_bits(q.get_state(), st_r)
    q.reset()
    q.run(tr_.win)
    assert same_bits(q.read_q8(), u8)   # and the int8 run after it is the int8 run before it
    for st in (h, r, a, q):
        st.close()


def check_calibrate_refusals(lib):
    for name in KERNEL_CASES:
        c = KernelCase(lib, name)
        tr_ = c.tracks()
        st = c.new()
        bad = tr_.win.copy()
        if c.stride > 1:
            bad[4]["copy_rows"] -= 1   # rows not a multiple of the stride
            with pytest.raises(native.NativeError, match=r"error -?\d+: calibration track 4 .*multiple of the stride 3"):
                st.calibrate(bad)
        with pytest.raises(native.NativeError, match="at least one track"):
            st.calibrate(tr_.win[:0])
        bad = tr_.win.copy()
        bad[2]["src_elem"] = 10 ** 12
        with pytest.raises(native.NativeError, match="past the end of its store"):
            st.calibrate(bad)
        # a refused call leaves the stream usable
        assert np.array_equal(st.calibrate(tr_.win)[1], c.new().calibrate_host(np.concatenate(tr_.frames)))
        st.close()
        if c.refused is not None:   # the creators without the int8 entry points answer as calibrate_host does
            old = c.new(c.refused)
            said = []
            for call in (lambda: old.calibrate_host(np.zeros((6, 40), np.float32)), lambda: old.calibrate(tr_.win)):
                with pytest.raises(native.NativeError) as e:
                    call()
                said.append(str(e.value))
            assert said[0] == said[1] and ("MixedNet streams only" in said[0] or "residual_connection" in said[0]), said
            off = np.zeros(tr_.win.size + 1, np.int64)
            ranges = np.zeros((4, 2), np.float32)
            rc = lib.lib.mww_stream_calibrate(old.h, native.vp(tr_.win), tr_.win.size, native.vp(off), native._fptr(ranges))
            assert rc == -3   # MWW_ERR_UNSUPPORTED
            old.close()
    # no weights yet
    c = KernelCase(lib, "plain-s1")
    st = c.new_raw()
    with pytest.raises(native.NativeError, match="set_weights"):
        st.calibrate(c.tracks().win)
    st.close()


# ------------------------------------------------------------------------------------------------- the calibration set
def host_rows(fh, windows):
    """the float32 rows the device serves for ``windows``, restated: zero rows for the padding, u16 values scaled"""
    where = {int(sid): (p, key) for p in fh.feature_providers if getattr(p, "flat", None) for key, sid in p.store_id.items()}
    parts = []
    for w in windows:
        p, key = where[int(w["store"])]
        a = p.flat[key][int(w["src_elem"]):int(w["src_elem"]) + int(w["copy_rows"]) * 40].reshape(-1, 40)
        parts += [np.zeros((int(w["pad_rows"]), 40), np.float32), a.astype(np.float32) * ec.SCALE if key == "u16" else a.astype(np.float32)]
    return np.concatenate(parts, 0)


def check_calibration_windows(lib):
    model, fh = mc.make_handler(lib)
    cfg1, cfg3 = dict(spectrogram_length=mc.T, stride=1), dict(spectrogram_length=63, stride=3)
    fh.use_private_rng(prefetch=0)
    private = [a.copy() for a in fh._private_rng]
    before = mc.rng_state()
    a = quantize.calibration_windows(fh, cfg1, 40, seed=0)
    b = quantize.calibration_windows(fh, cfg1, 40, seed=0)
    other = quantize.calibration_windows(fh, cfg1, 40, seed=1)
    c3 = quantize.calibration_windows(fh, cfg3, 40, seed=0)
    assert mc.same_rng(mc.rng_state(), before)
    assert all(np.array_equal(x, y) for x, y in zip(private, fh._private_rng))
    fh.release_private_rng()
    assert a.dtype == native.WINDOW_DTYPE and a.size == 40 and a.tobytes() == b.tobytes() and a.tobytes() != other.tobytes()
    assert np.all(a["pad_rows"] + a["copy_rows"] == mc.T - 1) and np.all(c3["pad_rows"] + c3["copy_rows"] == 60)
    assert np.all(a["pad_rows"] >= 0) and np.all(a["copy_rows"] >= 0) and len(set(a["store"].tolist())) > 1
    # the cut comes off the end: the drawn windows, one row (three rows) shorter
    drawn = fh.draw_seeded_windows(40, mc.T, 0)
    assert np.array_equal(drawn["store"], a["store"]) and np.array_equal(drawn["src_elem"], a["src_elem"])
    assert np.array_equal(drawn["pad_rows"], a["pad_rows"]) and np.array_equal(drawn["copy_rows"] - 1, a["copy_rows"])
    # ... which are the windows of a training draw from generators in that state
    saved = mc.rng_state()
    random.seed(0)
    np.random.seed(0)
    assert fh.draw_training_batch(40, mc.T)["windows"].tobytes() == drawn.tobytes()
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    assert np.array_equal(quantize.window_host_rows(fh, a), host_rows(fh, a))
    # a mined provider changes nothing
    src = fh.feature_providers[1]
    fh.add_mined_provider(np.array([(src.store_id["u16"], 0, 70, 0, 40 * 3)], native.WINDOW_DTYPE), sampling_weight=50.0)
    assert quantize.calibration_windows(fh, cfg1, 40, seed=0).tobytes() == a.tobytes()
    with pytest.raises(ValueError, match="multiple of the stride"):
        quantize.calibration_windows(fh, dict(spectrogram_length=mc.T, stride=7), 8)


# ------------------------------------------------------------------------------------------------- the loop
SVQ = dict(svc.SV, quantized=True, calibration_samples=8)
MINING_Q = dict(smc.MINING, quantized=True, calibration_samples=8)


def mixednet_model(lib, flags=ec.DEF, seed=7):
    from microwakeword_amd import mixednet
    return mixednet.model(flags, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=seed, max_batch=64)


def restated_model(model, fh, cfg, samples=8, seed=0):
    """the int8 model of ``model``'s weights by the host path: the float stream of its family, fresh, ``calibrate_host`` on the
    host rows of the calibration windows, the input range widened, the family's ``quantize``"""
    from microwakeword_amd.layout import InceptionLayout
    graph = isinstance(model.layout, InceptionLayout)
    module = quantize_graph if graph else quantize_mixednet if streaming.mixednet_variant_flags(model.flags) else quantize
    windows = quantize.calibration_windows(fh, dict(cfg, stride=1) if graph else cfg, samples, seed)
    assert np.all(windows["pad_rows"] + windows["copy_rows"] == cfg["spectrogram_length"] - (1 if graph else cfg["stride"]))
    if module is quantize:
        st = streaming.StreamingModel(model, int(cfg["stride"]), "stream").native
    else:
        st = (native.GraphStream if graph else native.Stream)(model.engine, module._description(model), int8=True)
        st.set_weights(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in model.get_weights()]))
    ranges = st.calibrate_host(host_rows(fh, windows))
    st.close()
    ranges[0, 0], ranges[0, 1] = min(ranges[0, 0], np.float32(0.0)), max(ranges[0, 1], np.float32(26.0))
    return module.quantize(model, ranges)


def restated(lib, cfg, weights=None, model=None):
    """the streaming metrics of the int8 model of a fresh model (the run's initial weights, or a weights file of the run) by the
    host restatement; also the int8 and the float probabilities"""
    v = streaming.streaming_validation_config(cfg)
    random.seed(1)
    np.random.seed(1)
    fresh = model if model is not None else mixednet_model(lib)
    if weights is not None:
        fresh.load_weights(weights)
    fh = FeatureHandler(cfg, engine=fresh.engine)
    qm = restated_model(fresh, fh, cfg, v["calibration_samples"], v["calibration_seed"])
    stride = int(qm.desc["stride"])
    sm = streaming.QuantizedStreamingModel(qm, stride, v["mode"], context=fresh)
    amb, _ = fh.track_windows(v["ambient_set"], sm.frames)
    pos, _ = fh.track_windows(v["data_set"], sm.frames, only_label=1.0)
    sm.reset()
    off = sm.native.run(np.concatenate([amb, pos]))
    p = sm.read_probabilities()
    fm = streaming.StreamingModel(fresh, stride, v["mode"])
    fm.native.run(np.concatenate([amb, pos]))
    tracks = [p[off[t]:off[t + 1]] for t in range(off.size - 1)]
    host = streaming.operating_summary_host(tracks[:amb.size], tracks[amb.size:], v["windows"], streaming.CUTOFFS, sm.stride,
                                            cfg["window_step_ms"] / 1000, v["ignore_slices_after_accept"], v["target_faph"])
    return streaming.streaming_metrics(host), p, fm.read_probabilities()


def int8_lines(caplog):
    return [r.getMessage() for r in caplog.records if "(streaming" in r.getMessage()]


def check_restatement(lib, tmp_path, caplog):
    """the line logged at step 0 and at every boundary is the restatement at that boundary's weights"""
    import logging
    cfg = svc.config(tmp_path, "q", SVQ)
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        smc.run_loop(lib, cfg)
    lines = svc.log_of(cfg, "validation_streaming")
    assert [e["step"] for e in lines] == [0] + svc.BOUNDARIES
    said = int8_lines(caplog)
    assert len(said) == 4 and all("(streaming, int8)" in s for s in said), said
    differs = False
    for line in lines:
        metrics, p_q, p_f = restated(lib, cfg, svc.weights_at(cfg, line["step"]) if line["step"] else None)
        svc.same_metrics(line, metrics, line["step"])
        assert p_q.shape == p_f.shape
        differs |= not np.array_equal(p_q, p_f)
    assert differs   # the restatement is not the float stream's
    return cfg


def check_float_log_line(lib, tmp_path, caplog):
    """a float validation's log line and scalars entry gain nothing"""
    import logging
    cfg = svc.config(tmp_path, "f", svc.SV, training_steps=[4, 0])
    with caplog.at_level(logging.INFO, logger="microwakeword_amd.train"):
        smc.run_loop(lib, cfg)
    said = int8_lines(caplog)
    assert said and all(s.split(":")[0].endswith("(streaming)") and "int8" not in s for s in said), said
    assert all(set(e) == set(streaming.STREAMING_METRICS) | {"step"} for e in svc.log_of(cfg, "validation_streaming"))


def check_unnamed_changes_nothing(lib, tmp_path):
    """the quantized keys present, the best-weights rule naming no streaming metric: the run without the mapping, byte for byte"""
    cfg_a, cfg_q = svc.config(tmp_path, "a"), svc.config(tmp_path, "q", SVQ)
    model_a, _ = smc.run_loop(lib, cfg_a)
    state_a, opt_a = [w.tobytes() for w in model_a.get_weights()], model_a.engine.get_opt_state()
    model_q, _ = smc.run_loop(lib, cfg_q)
    opt_q = model_q.engine.get_opt_state()
    assert state_a == [w.tobytes() for w in model_q.get_weights()]
    assert opt_a[0].tobytes() == opt_q[0].tobytes() and opt_a[1].tobytes() == opt_q[1].tobytes() and opt_a[2] == opt_q[2] == smc.STEPS
    for which in ("validation", "train"):
        assert svc.log_bytes(cfg_a, which) == svc.log_bytes(cfg_q, which)
    for name in ("last_weights.weights.h5", "best_weights.weights.h5", os.path.join("restore", "ckpt.weights")):
        assert svc.file_arrays(os.path.join(cfg_a["train_dir"], name)) == svc.file_arrays(os.path.join(cfg_q["train_dir"], name)), name
    assert [e["step"] for e in svc.log_of(cfg_q, "validation_streaming")] == [0] + svc.BOUNDARIES


def check_selection_follows_int8(lib, tmp_path):
    """with the streaming metric names, best_weights is the boundary the int8 metrics prefer"""
    cfg = svc.config(tmp_path, "n", SVQ, **svc.STREAMING_NAMES)
    smc.run_loop(lib, cfg)
    lines = [e for e in svc.log_of(cfg, "validation_streaming") if e["step"]]
    names = svc.STREAMING_NAMES
    entries = []
    for e in lines:   # the int8 metrics, restated
        m = restated(lib, cfg, svc.weights_at(cfg, e["step"]))[0]
        svc.same_metrics(e, m, e["step"])
        entries.append((e["step"], m[names["minimization_metric"]], m[names["maximization_metric"]]))
    best_step = svc.preferred(entries, names["target_minimization"])
    assert best_step in svc.BOUNDARIES
    assert svc.file_arrays(os.path.join(cfg["train_dir"], "best_weights.weights.h5")) == svc.file_arrays(svc.weights_at(cfg, best_step))


class CountedCalibrations:
    """counts the calls of native.Stream.calibrate while it is active"""

    def __init__(self, monkeypatch):
        self.calls = 0
        real = native.Stream.calibrate

        def counted(st, windows):
            self.calls += 1
            return real(st, windows)
        monkeypatch.setattr(native.Stream, "calibrate", counted)


def check_mining_quantized(lib, tmp_path, monkeypatch):
    """the first round's clips are mine_hard_negatives_on_device with the restated int8 model; with both mappings quantized one
    calibration per boundary"""
    cfg = smc.loop_config(tmp_path, "mq", MINING_Q)
    cfg["training_steps"] = [6, 2]   # one round, at step 4
    counter = CountedCalibrations(monkeypatch)
    smc.run_loop(lib, cfg)
    assert counter.calls == 1 and [int(e["step"]) for e in smc.mining_log(cfg)] == [4]
    z = smc.mined_file(cfg)
    random.seed(1)
    np.random.seed(1)
    fresh = mixednet_model(lib, seed=99)
    fresh.load_weights(svc.weights_at(dict(cfg), 4))
    fh = FeatureHandler(cfg, engine=fresh.engine)
    qsm = streaming.QuantizedStreamingModel(restated_model(fresh, fh, cfg), int(cfg["stride"]), "stream", context=fresh)
    by_hand, rep = mining.mine_hard_negatives_on_device(qsm, fh, 0.0, max_new=7, ignore_slices_after_accept=5)
    assert by_hand.size > 0 and smc.file_rows(z) == smc.rows_of(by_hand, fh), (smc.file_rows(z), smc.rows_of(by_hand, fh))
    assert smc.mining_log(cfg)[0]["detections"] == rep["detections"]
    # both quantized: the dry validation and the boundaries 4, 8, 12 calibrate once each (the rounds at 4 and 8 take the cached model)
    counter.calls = 0
    cfg_b = svc.config(tmp_path, "both", SVQ, dict(MINING_Q, sampling_weight=0.0))
    smc.run_loop(lib, cfg_b)
    assert counter.calls == 4 and [int(e["step"]) for e in smc.mining_log(cfg_b)] == [4, 8]
    # at sampling weight 0 the validation lines are those of the run without mining
    cfg_q = svc.config(tmp_path, "q", SVQ)
    smc.run_loop(lib, cfg_q)
    assert svc.log_bytes(cfg_b, "validation_streaming") == svc.log_bytes(cfg_q, "validation_streaming")


def check_draws_nothing(lib):
    """construction draws from the seeded states only, a validation and a round from none"""
    cfg = dict(ec.learnable_config(T=smc.T_LOOP), spectrogram_length=smc.T_LOOP, train_dir="unused")
    model = mixednet_model(lib)
    fh = FeatureHandler(cfg, engine=model.engine)
    before = mc.rng_state()
    state = streaming.StreamingValidation(streaming.streaming_validation_config(dict(streaming_validation=SVQ)), model, fh, cfg)
    rounds = mining.MiningRounds(mining.mining_config(dict(hard_negative_mining=MINING_Q)), model, fh, cfg, quantizer=state.quantizer)
    assert rounds.quantizer is state.quantizer and state.quantizer.windows.size == 8
    first = state.validate(0)
    rounds.round(0)
    assert mc.same_rng(mc.rng_state(), before) and state.quantizer.calibrations == 1
    assert state.validate(0) == first and set(first) == set(streaming.STREAMING_METRICS)
    # a non-finite calibrated range fails with a ValueError that names the key
    weights = model.get_weights()
    model.set_weights([np.full_like(w, np.nan) for w in weights])
    with pytest.raises(ValueError, match="streaming_validation: quantized: .*not finite"):
        state.validate(1)
    model.set_weights(weights)


def check_refusals(lib, tmp_path, monkeypatch):
    from microwakeword_amd import model_train_eval
    conf, mconf = streaming.streaming_validation_config, mining.mining_config
    for bad, word in ((dict(calibration_samples=0), "calibration_samples"), (dict(calibration_samples=2.5), "calibration_samples"),
                      (dict(calibration_samples="many"), "calibration_samples"), (dict(calibration_seed=-1), "calibration_seed"),
                      (dict(calibration_seed="x"), "calibration_seed"), (dict(quantized="yes"), "quantized"), (dict(quantised=True), "quantised")):
        with pytest.raises(ValueError, match="streaming_validation.*" + word):
            conf(dict(streaming_validation=dict(svc.SV, **bad)))
        with pytest.raises(ValueError, match="hard_negative_mining.*" + word):
            mconf(dict(hard_negative_mining=dict(smc.MINING, **bad)))
    v = conf(dict(streaming_validation=dict(svc.SV, quantized=True)))
    assert (v["quantized"], v["calibration_samples"], v["calibration_seed"]) == (True, 500, 0)
    m = mconf(dict(hard_negative_mining=dict(smc.MINING, calibration_seed=3)))
    assert (m["quantized"], m["calibration_samples"], m["calibration_seed"]) == (False, 500, 3)
    model = mixednet_model(lib)

    def refused(cfg, error, word, who=model):
        with pytest.raises(error, match=word):
            tr.train(who, cfg, FeatureHandler(cfg, engine=who.engine), verbose=False)
        assert who.engine.get_opt_state()[2] == 0 and not os.path.exists(cfg["train_dir"])

    refused(svc.config(tmp_path, "samples", dict(SVQ, calibration_samples=0)), ValueError, "streaming_validation.*calibration_samples")
    refused(svc.config(tmp_path, "disagree", SVQ, dict(MINING_Q, calibration_seed=5)), ValueError, "disagree on calibration_samples")
    attentive = mixednet_model(lib, dict(ec.DEF, spatial_attention=1))
    refused(svc.config(tmp_path, "attention", dict(SVQ, mode="non_stream")), NotImplementedError, "spatial_attention", attentive)
    refused(smc.loop_config(tmp_path, "attention_m", dict(MINING_Q, mode="non_stream")), NotImplementedError, "spatial_attention", attentive)
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    refused(svc.config(tmp_path, "world", SVQ), ValueError, "streaming_validation.*world size 2")
    refused(smc.loop_config(tmp_path, "world_m", MINING_Q), ValueError, "hard_negative_mining.*world size 2")
    monkeypatch.undo()
    # the command line: before train_dir is claimed (and before a model is built)
    import yaml
    train_dir = tmp_path / "cli_run"
    base = dict(train_dir=str(train_dir), clip_duration_ms=1490, batch_size=smc.B_LOOP, features=[])
    argv = ["--training_config", str(tmp_path / "training_parameters.yaml"), "--train", "1", "mixednet"]
    attention = ["--spatial_attention", "1", "--residual_connection", "0,0,0,0"]
    for extra, flags, error, word in (
            (dict(streaming_validation=dict(SVQ, calibration_samples=0)), [], ValueError, "streaming_validation.*calibration_samples"),
            (dict(hard_negative_mining=dict(MINING_Q, calibration_samples=-3)), [], ValueError, "hard_negative_mining.*calibration_samples"),
            (dict(streaming_validation=dict(SVQ), hard_negative_mining=dict(MINING_Q, calibration_samples=9)), ["--residual_connection", "0,0,0,0"], ValueError,
             "disagree on calibration_samples"),
            (dict(streaming_validation=dict(SVQ, mode="non_stream")), attention, NotImplementedError, "spatial_attention"),
            (dict(hard_negative_mining=dict(MINING_Q, mode="non_stream")), attention, NotImplementedError, "spatial_attention")):
        with open(tmp_path / "training_parameters.yaml", "w") as out:
            yaml.safe_dump(dict(base, **extra), out)
        with pytest.raises(error, match=word):
            model_train_eval.main(argv + flags)
        assert not train_dir.exists()
    monkeypatch.setattr(tr, "process_group", lambda: (0, 2))
    with open(tmp_path / "training_parameters.yaml", "w") as out:
        yaml.safe_dump(dict(base, streaming_validation=dict(SVQ)), out)
    with pytest.raises(ValueError, match="streaming_validation.*world size 2"):
        model_train_eval.main(argv)
    assert not train_dir.exists()


def check_families(lib, tmp_path, family):
    """one quantized dry validation of an Inception model / a residual MixedNet equals its restatement"""
    from microwakeword_amd import inception
    cfg = svc.config(tmp_path, family, SVQ)
    if family == "inception":
        cfg["stride"] = 1
        make = lambda: inception.model(ec.INC, (smc.T_LOOP, 40), smc.B_LOOP, lib=lib, seed=7, max_batch=64)   # noqa: E731
    else:
        make = lambda: mixednet_model(lib, dict(ec.DEF, residual_connection="0,1,0,1"))   # noqa: E731
    random.seed(1)
    np.random.seed(1)
    model = make()
    fh = FeatureHandler(cfg, engine=model.engine)
    state = streaming.StreamingValidation(streaming.streaming_validation_config(cfg), model, fh, cfg)
    assert state.quantizer.module is (quantize_graph if family == "inception" else quantize_mixednet)
    got = state.validate(0)
    want, p_q, p_f = restated(lib, cfg, model=make())
    assert set(got) == set(want) and all(got[k] == float(want[k]) or (got[k] != got[k] and want[k] != want[k]) for k in got), (got, want)
    assert not np.array_equal(p_q, p_f)
