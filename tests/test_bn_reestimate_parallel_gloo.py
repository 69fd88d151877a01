"""BatchNorm re-estimation under data parallelism (gloo, world size 2, the product kernels host-emulated under tests/hipemu, as in
tests/test_weight_ema_parallel_gloo.py): with rank-local BatchNorm every rank passes over windows of its own shard, and the ranks
end the boundary with byte-equal ``ema_bn`` - ``averaging.bn_rank_mean`` of the two shard results."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_parallel_gloo import _free_port

T, STEPS, LR, DECAY, K = 60, 3, 1e-3, 0.9, 2


def _worker(rank, world, port, out_dir, emu_path):
    import ctypes as C

    import engine_checks as ec
    from microwakeword_amd import native
    from microwakeword_amd.parallel import DataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    lib = native.NativeLib(emu_path)
    z = np.load(os.path.join(out_dir, "inputs.npz"))
    Bl = z["x"].shape[1] // world

    def wrap(ptr, n):   # emulated "device" memory is host memory
        return torch.from_numpy(np.ctypeslib.as_array((C.c_float * n).from_address(ptr)))

    lay, eng = ec.make_engine(lib, T, Bl, ec.perturbed_oracle(T))
    g = wrap(eng.device_ptr(native.BUF_GRADS), eng.n_params)
    p = wrap(eng.device_ptr(native.BUF_PARAMS), eng.n_params)
    dp = DataParallel(eng, g, p, None, sync_bn=False, wrap=wrap)
    assert dp.world == world
    eng.set_weight_ema(DECAY, 1)
    for s in range(STEPS):
        eng.set_batch(z["x"][s, rank * Bl:(rank + 1) * Bl])
        eng.set_targets(z["y"][s, rank * Bl:(rank + 1) * Bl], z["w"][s, rank * Bl:(rank + 1) * Bl])
        dp.train_step(Bl, LR)
    # the boundary: a pass over K batches of this rank's shard, then the ranks' mean
    eng.bn_reestimate_begin()
    for k in range(K):
        eng.set_batch(z["px"][k, rank * Bl:(rank + 1) * Bl])
        eng.bn_reestimate_batch(Bl)
    eng.bn_reestimate_commit()
    mine, valid = eng.get_ema_bn_state()
    assert valid
    dp.average_ema_bn_state()
    final, valid = eng.get_ema_bn_state()
    assert valid
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mine=mine, final=final, ema=eng.get_ema_state()[0], state=eng.get_bn_state())
    # the next update of the average invalidates on every rank alike
    eng.set_batch(z["x"][0, rank * Bl:(rank + 1) * Bl])
    eng.set_targets(z["y"][0, rank * Bl:(rank + 1) * Bl], z["w"][0, rank * Bl:(rank + 1) * Bl])
    dp.train_step(Bl, LR)
    assert not eng.ema_bn_valid()
    eng.close()
    dist.destroy_process_group()


def test_two_ranks_end_a_boundary_with_the_mean_of_their_shard_results(tmp_path):
    import conftest
    import engine_checks as ec
    from microwakeword_amd import averaging
    emu = conftest.build_emulator_lib()
    if emu is None:
        pytest.skip("clang++ not available for the host-side emulator build")
    W, Bl = 2, 3
    rng = np.random.default_rng(3)
    x = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(STEPS)])
    px = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(K)])
    y = (rng.random((STEPS, W * Bl)) < 0.5).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=(STEPS, W * Bl)).astype(np.float32)
    np.savez(tmp_path / "inputs.npz", x=x, y=y, w=w, px=px)
    mp.spawn(_worker, args=(W, _free_port(), str(tmp_path), emu), nprocs=W, join=True)
    a, b = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(W))
    assert a["ema"].tobytes() == b["ema"].tobytes()            # the same averaged weights ...
    assert a["mine"].tobytes() != b["mine"].tobytes()          # ... other shards, other statistics
    assert a["final"].tobytes() == b["final"].tobytes()
    want = averaging.bn_rank_mean([a["mine"], b["mine"]])
    assert a["final"].tobytes() == want.tobytes()
    assert a["final"].tobytes() != a["state"].tobytes()        # not the master's moving statistics
