"""Weight averaging under data parallelism (gloo, world size 2, the product kernels host-emulated under tests/hipemu, as in
tests/test_weight_qat_parallel_gloo.py): with sync-BN and the overlapped two-bucket gradient exchange the update sits behind the
Adam it follows, nothing is reduced, and both ranks end with byte-equal averages - the restatement over rank 0's masters."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_parallel_gloo import _free_port

T, STEPS, LR, DECAY, EVERY = 60, 4, 1e-3, 0.9, (1, 2)


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

    for every in EVERY:
        lay, eng = ec.make_engine(lib, T, Bl, ec.perturbed_oracle(T))
        g = wrap(eng.device_ptr(native.BUF_GRADS), eng.n_params)
        p = wrap(eng.device_ptr(native.BUF_PARAMS), eng.n_params)
        dp = DataParallel(eng, g, p, None, sync_bn=True, wrap=wrap, grad_buckets=2)
        assert dp.world == world
        eng.set_weight_ema(DECAY, every)
        masters = []
        for s in range(STEPS):
            eng.set_batch(z["x"][s, rank * Bl:(rank + 1) * Bl])
            eng.set_targets(z["y"][s, rank * Bl:(rank + 1) * Bl], z["w"][s, rank * Bl:(rank + 1) * Bl])
            dp.train_step(Bl, LR)
            masters.append(eng.get_params())
        ema, updates = eng.get_ema_state()
        np.savez(os.path.join(out_dir, "every%d_rank%d.npz" % (every, rank)), masters=np.stack(masters), ema=ema, updates=updates,
                 step=eng.get_opt_state()[2])
        eng.close()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_average_and_it_is_the_restatement(tmp_path):
    import conftest
    import engine_checks as ec
    from microwakeword_amd import averaging
    emu = conftest.build_emulator_lib()
    if emu is None:
        pytest.skip("clang++ not available for the host-side emulator build")
    W, Bl = 2, 3
    rng = np.random.default_rng(3)
    x = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(STEPS)])
    y = (rng.random((STEPS, W * Bl)) < 0.5).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=(STEPS, W * Bl)).astype(np.float32)
    np.savez(tmp_path / "inputs.npz", x=x, y=y, w=w)
    mp.spawn(_worker, args=(W, _free_port(), str(tmp_path), emu), nprocs=W, join=True)
    for every in EVERY:
        a, b = (np.load(tmp_path / ("every%d_rank%d.npz" % (every, r))) for r in range(W))
        assert int(a["step"]) == int(b["step"]) == STEPS and int(a["updates"]) == int(b["updates"]) == STEPS // every
        assert a["masters"].tobytes() == b["masters"].tobytes()
        assert a["ema"].tobytes() == b["ema"].tobytes()   # nothing was reduced: the same function of identical masters
        want, n = averaging.ema_fold(list(a["masters"]), DECAY, every)
        assert n == STEPS // every and a["ema"].tobytes() == want.tobytes()
        assert a["ema"].tobytes() != a["masters"][-1].tobytes()
