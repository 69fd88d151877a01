"""W > 1 data-parallel steps through the replay rendezvous of tests/exchange_replay.py on the host-emulated kernels
(tests/hipemu): (a) the harness itself against a real two-process gloo all-reduce, bit for bit, and a fixed slice of the cases
tests/test_exchange_replay_gpu.py runs on the MI355X (tests/exchange_checks.py).  The slice is the one every mutation of the
exchange listed in profiles/exchange_replay_results.txt fails."""
import numpy as np
import pytest
import torch.multiprocessing as mp

import block_table_sweep as bts
import engine_checks as ec
import exchange_checks as xc
import graph_table_sweep as gts
from exchange_replay import replay
from microwakeword_amd import native
from test_parallel_gloo import T, _free_port, _sync_worker

SETTINGS = ((True, 1), (False, 1), (False, 2))   # (sync-BN, gradient buckets)


def _gloo_workers(rank, world, ports, out_dir, emu_path, kind):
    for (sync, buckets), port in zip(SETTINGS, ports):
        _sync_worker(rank, world, port, out_dir, emu_path, kind, sync, buckets, "s%db%d_" % (sync, buckets))


@pytest.mark.parametrize("kind", ["mixednet", "inception", "graph_mixednet"])
def test_replay_equals_a_two_process_gloo_all_reduce(emu_lib, tmp_path, kind):
    """(a) test_parallel_gloo._sync_worker on two processes against the replay of the same step in this one: gradients,
    parameters and BN state bit for bit, under sync-BN and in throughput mode with 1 and 2 buckets."""
    import conftest
    from microwakeword_amd.layout import GraphMixedNetLayout, InceptionLayout, MixedNetLayout
    W, Bl = 2, 3
    rng = np.random.default_rng(3)
    x, y, w = xc.batch(rng, W * Bl, T)
    if kind == "inception":
        om, lay = ec.perturbed_inception_oracle(T, ec.INC), InceptionLayout(ec.INC, T)
        keep = (rng.random((W * Bl, lay.t_last * lay.c_last)) >= ec.INC["dropout"]).astype(np.float32)
    elif kind == "mixednet":
        om, lay, keep = ec.perturbed_oracle(T), MixedNetLayout(ec.DEF, T), None
    else:
        om, lay, keep = ec.perturbed_oracle(T, flags=ec.GRAPH_MIXEDNET), GraphMixedNetLayout(ec.GRAPH_MIXEDNET, T), None
    np.savez(tmp_path / "inputs.npz", x=x, y=y, w=w, keep=keep if keep is not None else np.zeros(1))
    ports = [_free_port() for _ in SETTINGS]
    mp.spawn(_gloo_workers, args=(W, ports, str(tmp_path), conftest.EMU, kind), nprocs=W, join=True)
    p0, s0 = lay.pack(om.get_weights())
    for sync, buckets in SETTINGS:
        def make_rank(r):
            eng = native.Engine(lib=emu_lib, **lay.engine_args(Bl))
            if kind != "inception":
                eng.set_grad_mask(lay.grad_mask())
            eng.set_params(p0)
            eng.set_bn_state(s0)
            eng.set_option("grad_buckets", buckets)
            return eng

        def script(eng, r):
            xc._step(eng, Bl, r, x, y, w, keep)
            return dict(grads=eng.get_grads(), params=eng.get_params(), state=eng.get_bn_state())

        got, ex = replay(W, make_rank, script, sync_bn=sync)
        for r in range(W):
            want = np.load(tmp_path / ("s%db%d_%d.npz" % (sync, buckets, r)))
            assert ex.calls == [tuple(c) for c in want["exchanges"].tolist()], (ex.calls, want["exchanges"])
            for k in ("grads", "params", "state"):
                assert got[r][k].tobytes() == want[k].tobytes(), "%s sync %d buckets %d rank %d: %s differ by %.3g" % (
                    kind, sync, buckets, r, k, np.abs(got[r][k] - want[k]).max())


def test_sync_bn_block_engine_slice(emu_lib):
    """(b) one case per (mode, bwd_wide, first-block backward form) of the block sweep at W = 2, the default topology at
    W = 3, and one with fewer windows per rank than the grid."""
    cases = xc.block_cases(emu_lib)
    forms = set().union(*(c["forms"] for c in cases if c["forms"]))
    assert forms == set().union(*(bts.case_forms(c) for c in bts.plan(emu_lib))), "the GPU list misses a form of the block sweep"
    for c in xc.block_slice(cases):
        try:
            xc.report(c["id"], xc.check_sync_bn_block(emu_lib, c))
        except AssertionError as e:
            raise AssertionError("%s (T %d, W %d x %d windows, grid %d): %s" % (c["id"], c["T"], c["W"], c["Bl"], c["grid"], e)) from None


def test_declared_graph_kernels():
    """The graph cases run, by graph_table_sweep's restatement of a sync-BN rank's route, the two instantiations its own sweep
    cannot reach - and nothing outside the library's inventory."""
    ks = xc.declared_graph_kernels()
    assert {"gconv_bwd_kernel<10, 10, GSh3>", "gconv_bwd_kernel<16, 16, GSh7>"} <= ks
    assert {"gconv_bwd_kernel<10, 10, GSh3>", "gconv_bwd_kernel<16, 16, GSh7>"} <= set(gts.UNREACHABLE)
    assert ks <= set(gts.inventory()), sorted(ks - set(gts.inventory()))
    assert not any(k.startswith(("gconv_fwd2", "gconv_bwd2")) for k in ks)   # pairing off


@pytest.mark.parametrize("cid", xc.GRAPH_SLICE)
def test_sync_bn_graph_engine_slice(emu_lib, cid):
    case = [c for c in xc.graph_cases() if c["id"] == cid][0]
    xc.report(cid, xc.check_sync_bn_graph(emu_lib, case))


@pytest.mark.parametrize("kind", ["mixednet", "inception"])
def test_throughput_mode_is_a_composition_of_single_device_pieces(emu_lib, kind):
    xc.report("throughput-" + kind, xc.check_throughput_composition(emu_lib, kind))


def test_step_features_behind_the_exchange(emu_lib):
    """(d) at the emulator's pace: one QAT step, two steps of the average, and the re-estimation
    (the GPU file runs three and four steps, and the average at both cadences)."""
    xc.report("weight-qat-1-step", xc.check_weight_qat(emu_lib, steps=1))
    xc.report("weight-ema-2-steps", xc.check_weight_ema(emu_lib, steps=2, every_steps=(1,)))
    xc.report("bn-reestimate-sync-bn", xc.check_bn_reestimate_sync(emu_lib))
