"""Streaming evaluation of MixedNets with residual connections, a pooled head or spatial attention (stream_forward_kernel<true, *> of csrc/tu_stream.hip,
mww_stream_create_mixednet) under the host-side emulator of tests/hipemu: every case of tests/mixednet_variant_checks.py,
the reference-graph fixture, the refusals of the ABI and ``StreamingModel`` on such models."""
import numpy as np
import pytest

import engine_checks as ec
import mixednet_variant_checks as vc
import mixednet_variant_streaming_oracle as vo
import streaming_checks as sc
from microwakeword_amd import streaming


@pytest.mark.parametrize("cid", vc.case_ids())
def test_case_matches_the_oracles(emu_lib, cid):
    res = vc.run_case(emu_lib, vc.case(cid), n_cu=4)   # the emulated device has 4 CUs
    print("[mixednet_variant] %s" % res, flush=True)


def test_reference_graph_fixture(emu_lib, golden_dir):
    vc.check_reference_fixture(emu_lib, golden_dir)


def test_abi_refusals(emu_lib):
    vc.check_abi_refusals(emu_lib)


def test_pool_with_one_final_frame_is_the_plain_stream(emu_lib):
    """pool on a description with t_final = 1 through the new creator: the bits of mww_stream_create, int8 entry points open"""
    from microwakeword_amd import native
    b = vc.built("pooled-flags_tf1_plain")
    model = sc.context_model(emu_lib)
    plain = {k: v for k, v in b.desc.items() if k not in ("residual", "attention", "pool")}
    outs = []
    for d in (b.desc, plain):
        st = native.Stream(model.engine, d)
        st.set_weights(b.flat)
        st.run_host(b.seq[:300])
        outs.append((st.read(), st.get_state(), st.num_tensors()))
        st.close()
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32)) and outs[0][2] == outs[1][2]


def test_streaming_model_closes_the_pooled_hole(emu_lib):
    """a pooled model through StreamingModel in stream mode: today's code scores the un-pooled Dense of the latest frame"""
    flags, T = dict(ec.GRAPH_MIXEDNET, pooled=1, residual_connection="1,0,1"), 31
    om, model = sc.make_model(emu_lib, flags, T)
    assert model.layout.t_last == 1
    sm = streaming.StreamingModel(model, int(flags["stride"]), "stream")
    assert sm.desc["t_final"] == vo.t_final_of(flags, T) > 1 and sm.desc["pool"] == "average"
    net = vo.Net(flags, om, T)
    tr = sc.Tracks(model, [0, 7, 2 * T + 3, 40], [0, 2, 0, 5], seed=4)
    off = sm.native.run(tr.win)
    p, z = sm.native.read(want_logits=True)
    s = net.s
    fed = np.concatenate([f[:(len(f) // s) * s] for f in tr.frames], 0)
    ref_z, ref_st = vo.whole_sequence(net, fed, rings=True)
    sc._compare(p, z, ref_z, "pooled StreamingModel")
    sc.compare_state(sm.native.get_state(), ref_st, net, "pooled StreamingModel")
    assert off[-1] == ref_z.size
    sc.check_predict_spectrogram_chunks(emu_lib, flags, T, [40, 3, 77, 0, 120])
    sc.check_non_stream_parity(emu_lib, flags, T, [T, T - 1, 0, T + 3 * s + 1], [T // 2, 0, 0, 0])
