"""Checks of the streaming evaluation (csrc/tu_stream.hip through microwakeword_amd.streaming) shared by the emulator tests
(tests/test_streaming_emulated.py, small sizes) and the GPU tests (tests/test_streaming_gpu.py, realistic sizes).  Every
check compares against the float64 restatement of tests/streaming_oracle.py."""
import numpy as np

from microwakeword_amd import mixednet, native, streaming
from microwakeword_amd.layout import GraphMixedNetLayout, MixedNetLayout
import engine_checks as ec
import streaming_oracle as so

PROB_TOL = 1e-5


def layout_of(flags, T):
    try:
        return MixedNetLayout(flags, T)
    except NotImplementedError:
        return GraphMixedNetLayout(flags, T)


def make_model(lib, flags, T, seed=42):
    om = ec.perturbed_oracle(T, seed=seed, flags=flags)
    model = mixednet.model(flags, (T, 40), 4, lib=lib, max_batch=64)
    model.set_weights(om.get_weights())
    return om, model


class Tracks:
    """Synthetic tracks in two resident stores of ``model.engine`` (u16 store 0, f32 store 1)."""

    def __init__(self, model, lengths, pads=None, seed=0, store_ids=(0, 1)):
        rng = np.random.default_rng(seed)
        self.lengths = list(lengths)
        self.pads = list(pads) if pads is not None else [0] * len(self.lengths)
        u16, f32, win, self.frames = [], [], [], []
        ou = of = 0
        for i, (L, pad) in enumerate(zip(self.lengths, self.pads)):
            rows = L - pad
            if i % 2 == 0:
                raw = rng.integers(0, 1200, size=(rows, 40)).astype(np.uint16)
                u16.append(raw.reshape(-1))
                win.append((store_ids[0], pad, rows, 0, ou))
                ou += raw.size
                x = raw.astype(np.float32) * np.float32(0.0390625)
            else:
                x = rng.uniform(0, 40, size=(rows, 40)).astype(np.float32)
                f32.append(x.reshape(-1))
                win.append((store_ids[1], pad, rows, 0, of))
                of += x.size
            self.frames.append(np.concatenate([np.zeros((pad, 40), np.float32), x], 0))
        u = np.concatenate(u16 + [np.zeros(40, np.uint16)])
        f = np.concatenate(f32 + [np.zeros(40, np.float32)])
        model.engine.upload_store(store_ids[0], u)
        model.engine.upload_store(store_ids[1], f)
        self.win = np.array(win, native.WINDOW_DTYPE).reshape(-1)


def stream_reference(om, flags, frames_list):
    """float64 logits of the streaming model fed the tracks in order from zero state, split per track"""
    net = so.Net(flags, om)
    s = net.s
    fed = [f[:(len(f) // s) * s] for f in frames_list]
    z = so.whole_sequence(net, np.concatenate(fed + [np.zeros((0, 40))], 0)) if sum(len(f) for f in fed) else np.zeros(0)
    out, at = [], 0
    for f in fed:
        n = len(f) // s
        out.append(z[at:at + n])
        at += n
    return out


def flags_of(desc):
    """the MixedNet flag set of a stream description (any the streaming plan accepts)"""
    return dict(ec.DEF, first_conv_filters=int(desc["conv1_filters"]), first_conv_kernel_size=int(desc["conv1_kernel"]),
                stride=int(desc["stride"]), pointwise_filters="".join("%d," % f for _, _, f in desc["blocks"]),
                repeat_in_block="".join("%d," % r for r, _, _ in desc["blocks"]),
                mixconv_kernel_sizes="".join("[%s]," % ",".join(str(int(k)) for k in ks) for _, ks, _ in desc["blocks"]),
                residual_connection="".join("0," for _ in desc["blocks"]))   # trailing commas: one block stays a list


def frames_of(desc):
    """window length T of the non-streaming model whose final map has desc["t_final"] frames ((T - k1) % stride == 0)"""
    sum_r = sum(int(r) * (max(ks) - 1) for r, ks, _ in desc["blocks"])
    return (int(desc["t_final"]) + sum_r - 1) * int(desc["stride"]) + int(desc["conv1_kernel"])


_CONTEXT = {}


def context_model(lib):
    """one small float model per library: native.Stream(model.engine, desc) runs any description in its context"""
    if id(lib) not in _CONTEXT:
        _CONTEXT[id(lib)] = (lib, make_model(lib, ec.DEF, 52)[1])
    return _CONTEXT[id(lib)][1]


def _compare(got_p, got_z, ref_z, what):
    ref_z = np.asarray(ref_z, np.float64)
    assert got_p.shape == ref_z.shape, (what, got_p.shape, ref_z.shape)
    if ref_z.size:
        assert np.abs(got_z - ref_z).max() <= ec.FWD_TOL, (what, np.abs(got_z - ref_z).max())
        assert np.abs(got_p - so.sigmoid(ref_z)).max() <= PROB_TOL, (what, np.abs(got_p - so.sigmoid(ref_z)).max())


def compare_state(got, ref, net, what):
    """``mww_stream_get_state`` against the oracle's rings: the conv1 ring is a copy of input frames (exact), every other
    ring holds plain activations (FWD_TOL).  Returns the largest activation-ring error."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    n1 = net.r1 * 40
    assert np.array_equal(got[:n1], ref[:n1].astype(np.float32)), (what, "conv1 ring differs")
    err = float(np.abs(got[n1:] - ref[n1:]).max()) if got.size > n1 else 0.0
    if not err <= ec.FWD_TOL:   # (a NaN fails too) name the first ring that is off: it localises the layer
        at, names = n1, ["mixconv %d" % i for i in range(len(net.ring_sizes()) - 2)] + ["head"]
        for name, n in zip(names, net.ring_sizes_flat()[1:]):
            e = float(np.abs(got[at:at + n] - ref[at:at + n]).max()) if n else 0.0
            assert e <= ec.FWD_TOL, (what, "ring of " + name, e)
            at += n
        raise AssertionError((what, "rings", err))
    return err


def check_stream_parity(lib, flags, T, calls, seed=0):
    """``calls``: list of (lengths, pads) run as successive mww_stream_run calls on one stream (state carried); the
    rings after every call are held to the oracle's as well."""
    om, model = make_model(lib, flags, T)
    sm = streaming.StreamingModel(model, int(flags["stride"]), "stream")
    net, s = so.Net(flags, om), int(flags["stride"])
    all_frames, got = [], []
    for ci, (lengths, pads) in enumerate(calls):
        tr = Tracks(model, lengths, pads, seed=seed + ci, store_ids=(2 * ci, 2 * ci + 1))
        off = sm.native.run(tr.win)
        p, z = sm.native.read(want_logits=True)
        assert off[-1] == p.size
        for t in range(len(lengths)):
            assert off[t + 1] - off[t] == lengths[t] // int(flags["stride"])
            got.append((p[off[t]:off[t + 1]], z[off[t]:off[t + 1]]))
        all_frames += tr.frames
        fed = np.concatenate([f[:(len(f) // s) * s] for f in all_frames] + [np.zeros((0, 40), np.float32)], 0)
        compare_state(sm.native.get_state(), so.whole_sequence(net, fed, rings=True)[1], net, "state after call %d" % ci)
    ref = stream_reference(om, flags, all_frames)
    for i, ((p, z), r) in enumerate(zip(got, ref)):
        _compare(p, z, r, "track %d" % i)
    return om, model, sm


def check_non_stream_parity(lib, flags, T, lengths, pads, seed=0, against_model=True):
    om, model = make_model(lib, flags, T)
    sm = streaming.StreamingModel(model, int(flags["stride"]), "non_stream")
    tr = Tracks(model, lengths, pads, seed=seed)
    off = sm.native.run(tr.win)
    p, z = sm.native.read(want_logits=True)
    s = int(flags["stride"])
    for t, f in enumerate(tr.frames):
        ref = so.non_stream_windows(om, f.astype(np.float64), T, s)
        _compare(p[off[t]:off[t + 1]], z[off[t]:off[t + 1]], ref, "track %d" % t)
        if against_model and ref.size:
            x = np.stack([f[e - T:e] for e in range(T, len(f) + 1, s)])
            pm = model.predict_on_batch(x).reshape(-1)
            assert np.abs(pm - p[off[t]:off[t + 1]]).max() <= PROB_TOL
    return sm


def check_metrics_kernel(sm, rng, n_tracks=6, max_len=400):
    """device moving average / cooldown counts / scores == the host restatement on the same probabilities, exactly"""
    lens = [int(v) for v in rng.integers(30, max_len, n_tracks)]
    probs = [np.clip(rng.random(n).astype(np.float32) ** 2 * 1.1, 0, 1).astype(np.float32) for n in lens]
    # values on and next to cutoffs
    probs[0][:60] = np.float32(0.37)
    probs[1][10:80] = np.nextafter(np.float32(0.5), np.float32(1))
    flat = np.concatenate(probs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    check_metrics_on(sm, flat, off, n_tracks)


def check_metrics_on(sm, flat, off, n_amb):
    """first n_amb tracks ambient, the rest positive"""
    sm.native.set_probs(flat)
    n = off.size - 1
    kind = np.array([0] * n_amb + [1] * (n - n_amb), np.int32)
    counts, ma_len, score = sm.metrics(off, kind)
    tracks = [flat[off[i]:off[i + 1]] for i in range(n)]
    mas = [streaming.moving_average(t) for t in tracks[:n_amb]]
    want = streaming.false_accept_counts(mas, streaming.CUTOFFS, 25)
    assert np.array_equal(counts, want), (counts, want)
    for i in range(n_amb):
        assert ma_len[i] == mas[i].size
    for i in range(n_amb, n):
        ma = streaming.moving_average(tracks[i][25:])
        assert ma_len[i] == ma.size
        if ma.size:
            assert score[i] == np.max(ma)


def check_predict_spectrogram_chunks(lib, flags, T, lengths, seed=3):
    """StreamingModel.predict_spectrogram called track by track == one predict_tracks-style run over the same tracks"""
    om, model = make_model(lib, flags, T)
    s = int(flags["stride"])
    a = streaming.StreamingModel(model, s, "stream")
    b = streaming.StreamingModel(model, s, "stream")
    tr = Tracks(model, lengths, seed=seed)
    off = a.native.run(tr.win)
    whole = a.read_probabilities()
    parts = [b.predict_spectrogram(f) for f in tr.frames]
    assert np.array_equal(np.concatenate(parts), whole)
    assert all(parts[i].size == off[i + 1] - off[i] for i in range(len(parts)))
    return whole
