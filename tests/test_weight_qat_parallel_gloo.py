"""Weight-only quantization-aware training under data parallelism (gloo, world size 2, the product kernels host-emulated under
tests/hipemu, as in tests/test_parallel_gloo.py): with the option on, sync-BN and the overlapped two-bucket gradient exchange,
both ranks hold byte-equal masters after three steps - every rank derives the same shadow from the same master - and that master
is the one a single rank reaches on the whole batch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_parallel_gloo import _free_port

T, STEPS, LR = 60, 3, 1e-3


def _worker(rank, world, port, out_dir, emu_path, tag):
    import ctypes as C

    import engine_checks as ec
    import weight_qat_checks as wq
    from microwakeword_amd import native, qat
    from microwakeword_amd.parallel import DataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    lib = native.NativeLib(emu_path)
    z = np.load(os.path.join(out_dir, "inputs.npz"))
    Bl = z["x"].shape[1] // world
    lay, eng = ec.make_engine(lib, T, Bl, ec.perturbed_oracle(T))

    def wrap(ptr, n):   # emulated "device" memory is host memory
        return torch.from_numpy(np.ctypeslib.as_array((C.c_float * n).from_address(ptr)))

    g = wrap(eng.device_ptr(native.BUF_GRADS), eng.n_params)
    p = wrap(eng.device_ptr(native.BUF_PARAMS), eng.n_params)
    dp = DataParallel(eng, g, p, None, sync_bn=True, wrap=wrap, grad_buckets=2)
    assert dp.world == world
    eng.set_weight_qat_map(*qat.channel_map(lay))
    eng.set_option("weight_qat", 1)
    for s in range(STEPS):
        eng.set_batch(z["x"][s, rank * Bl:(rank + 1) * Bl])
        eng.set_targets(z["y"][s, rank * Bl:(rank + 1) * Bl], z["w"][s, rank * Bl:(rank + 1) * Bl])
        dp.train_step(Bl, LR)
        wq.assert_shadow(eng, lay, "rank %d after step %d" % (rank, s + 1))
    m, v, step = eng.get_opt_state()
    np.savez(os.path.join(out_dir, "%s%d.npz" % (tag, rank)), params=eng.get_params(), state=eng.get_bn_state(), grads=eng.get_grads(),
             shadow=eng.get_forward_params(), m=m, v=v, step=step)
    eng.close()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_master_and_it_is_the_single_rank_s(tmp_path):
    import conftest
    import engine_checks as ec
    emu = conftest.build_emulator_lib()
    if emu is None:
        pytest.skip("clang++ not available for the host-side emulator build")
    W, Bl = 2, 3
    rng = np.random.default_rng(3)
    x = np.stack([ec.synth_x(rng, W * Bl, T) for _ in range(STEPS)])
    y = (rng.random((STEPS, W * Bl)) < 0.5).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=(STEPS, W * Bl)).astype(np.float32)
    np.savez(tmp_path / "inputs.npz", x=x, y=y, w=w)
    mp.spawn(_worker, args=(W, _free_port(), str(tmp_path), emu, "two"), nprocs=W, join=True)
    mp.spawn(_worker, args=(1, _free_port(), str(tmp_path), emu, "one"), nprocs=1, join=True)
    a, b, one = (np.load(tmp_path / name) for name in ("two0.npz", "two1.npz", "one0.npz"))
    assert int(a["step"]) == int(b["step"]) == int(one["step"]) == STEPS
    for k in ("params", "state", "grads", "shadow", "m", "v"):
        assert a[k].tobytes() == b[k].tobytes(), k   # byte-equal masters, statistics, optimizer state - and shadows
    assert not np.array_equal(a["shadow"], a["params"])
    # ... and the single rank's on the whole batch, under sync-BN the same step up to the order of the sums.  engine_checks holds
    # one engine step to 0.05 lr of the float64 step where the gradient is well away from zero (2 lr anywhere): two engine runs are
    # within twice that per step, over STEPS steps
    well = np.abs(one["grads"]) > 1e-4 * np.abs(one["grads"]).max()
    diff = np.abs(a["params"] - one["params"])
    print("world 2 against world 1 after %d steps: %.3g lr where well conditioned, %.3g lr anywhere" % (STEPS, diff[well].max() / LR, diff.max() / LR))
    assert diff[well].max() <= STEPS * 2 * 0.05 * LR and diff.max() <= STEPS * 2 * 2.0 * LR
    assert np.abs(a["state"] - one["state"]).max() <= STEPS * 2 * 1e-5 * max(1.0, np.abs(one["state"]).max())
