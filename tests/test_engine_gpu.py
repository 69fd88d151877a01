"""Parity tests proper: the HIP library (through the C ABI of include/mww.h) on a real MI355X
against oracle/ on identical seeded inputs.  Tolerances: integer/byte work (batch assembly,
SpecAugment indices, sampler) bit-exact; floating point within the north_star's 1e-3 on forward
outputs (tighter bounds on intermediates are stated in tests/engine_checks.py)."""
import os

import numpy as np
import pytest

import engine_checks as ec
from microwakeword_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    nl = native.NativeLib.get()  # raises loudly if libmww_hip.so is missing
    assert nl.device_count() >= 1, "no MI355X visible"
    return nl


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "data_golden.npz"))


def test_mfma_layout_probe(lib):
    """First thing on the GPU: a tiny forward whose only GEMMs are the MFMA tiles — a wrong lane
    map (cdna_hip_programming.md §3) would show here before anything else is interpreted."""
    err = ec.check_forward_parity(lib, B=1, T=60, training=False)
    assert err < 1e-4


@pytest.mark.parametrize("tag", ["u16", "f32"])
def test_get_data_reference_golden(lib, gold, tag):
    ec.check_get_data_against_reference_golden(lib, gold, tag)


def test_sampler_and_assemble_bit_exact(lib):
    ec.check_sampler_matches_oracle_descriptors(lib, B=256, n_samples=300)


@pytest.mark.parametrize("training", [False, True])
def test_forward_parity_small(lib, training):
    ec.check_forward_parity(lib, B=7, T=194, training=training)


def test_forward_parity_config2_batch1024(lib):
    """BASELINE config[1]: default mixednet, batch 1024, fp32, forward parity vs the CPU restatement."""
    assert ec.check_forward_parity(lib, B=1024, T=194, training=False) <= ec.FWD_TOL
    assert ec.check_forward_parity(lib, B=1024, T=194, training=True) <= ec.FWD_TOL


def test_forward_ragged_tiles(lib):
    ec.check_forward_parity(lib, B=3, T=111, training=True, grid=2)
    ec.check_forward_parity(lib, B=2, T=60, training=False)


def test_train_steps_small(lib):
    ec.check_train_steps(lib, B=6, T=194, steps=3, grid=0)
    ec.check_train_steps(lib, B=5, T=130, steps=1, grid=3)


def test_train_steps_graph_replay(lib):
    ec.check_train_steps(lib, B=6, T=194, steps=3, grid=0, graphs=True)


def test_train_step_batch64_multi_tile_grid(lib):
    ec.check_train_steps(lib, B=64, T=194, steps=1, grid=16)


def test_saturated_logits_loss_forms(lib):
    ec.check_saturated_logits_loss(lib, B=8, T=194)


def test_variable_batch_sizes_do_not_leave_stale_statistics(lib):
    ec.check_variable_batch_sizes(lib, T=194, sizes=(16, 4, 4, 1, 16))
    ec.check_variable_batch_sizes(lib, T=194, sizes=(16, 4, 4), graphs=True)


def test_train_step_at_the_baseline_size_vs_float64_oracle(lib):
    """BASELINE configs[1] size (B = 1024, T = 194: two windows per backward workgroup, every accumulator row contended):
    loss, probabilities, the whole flat gradient per tensor (L2 <= 1e-4), the Adam-updated weights, the BN moving
    statistics and the metric counters against one float64 oracle step (~20 s of CPU)."""
    worst = ec.check_train_steps(lib, B=1024, T=194, steps=1, grid=0)
    assert worst["l2_max"] <= 1e-4
    # ... and the same gradients without imposing the engine's ReLU decisions on the oracle
    assert ec.check_gradients_unimposed(lib, B=1024, T=194, bound=1e-2) <= 1e-2


def test_inception_train_step_batch1024_vs_float64_oracle(lib):
    ec.check_inception_train_steps(lib, B=1024, T=194, steps=1, grid=0)
    # ... and without imposing the engine's ReLU decisions on the oracle (a mask bug cannot hide)
    assert ec.check_gradients_unimposed(lib, B=1024, T=194, bound=2e-2, kind="inception") <= 2e-2


def test_notebook_topology_batch1024_gradients_without_imposed_masks(lib):
    """The topology the reference's notebook trains (first conv 5x1 stride 3, 64 filters, MixConv groups, T = 204) at B = 1024 on the
    kernels compiled for one workgroup per CU: train step vs the float64 oracle with and without the engine's ReLU decisions imposed."""
    worst = ec.check_train_steps(lib, B=1024, T=204, steps=1, grid=0, flags=ec.NOTEBOOK)
    assert worst["l2_max"] <= 1e-4
    assert ec.check_gradients_unimposed(lib, B=1024, T=204, bound=2e-2, flags=ec.NOTEBOOK) <= 2e-2


def test_gradients_without_imposed_masks_on_the_other_paths(lib):
    """The un-imposed check (nothing of the engine's ReLU decisions is copied into the oracle) for the paths that relied on
    the mask-imposing checks alone: a crossed block-kernel shape, a MixedNet on the generic graph kernels, and the
    bf16-operand mode (bounded by that mode's own float32-vs-float64 oracle noise)."""
    assert ec.check_gradients_unimposed(lib, B=1024, T=194, bound=2e-2, flags=ec.CROSSED[0]) <= 2e-2
    assert ec.check_gradients_unimposed(lib, B=512, T=204, bound=2e-2, flags=ec.CROSSED[4]) <= 2e-2
    assert ec.check_gradients_unimposed(lib, B=1024, T=194, bound=2e-2, kind="graph_mixednet") <= 2e-2
    ec.check_gradients_unimposed(lib, B=1024, T=194, bound=3e-2, flags=ec.BF16, noise_factor=3.0)


def test_gradients_without_imposed_masks_on_the_remaining_paths(lib):
    """... and for the three paths that still relied on mask-imposing checks alone (round-4 review): configs[4]'s full form
    (bf16 operands AND bf16 storage, bounded by the mode's own float32-vs-float64 oracle noise like the operand mode), the
    Inception variant with every flag away from its default (two stem layers, dilation 2, sub-spectral groups, dropout 0.3),
    and a MixedNet with residual branches, the attention gate and the pooled head on the graph kernels."""
    ec.check_gradients_unimposed(lib, B=1024, T=194, bound=3e-2, flags=ec.BF16_STORED, noise_factor=3.0)
    # (the variant's sub-spectral slots sum 8-12 channels into two values: some of those gradients nearly cancel - |ref| 7e-3 against
    # 0.27 for the largest tensor - and a handful of float32-vs-float64 ReLU flips then is 9 % of them; the bound of a tensor is
    # three times the float32 ORACLE's own distance from the float64 one, never below 2 %)
    ec.check_gradients_unimposed(lib, B=512, T=194, bound=2e-2, kind="inception", flags=ec.INC_VARIANT, noise_factor=3.0)
    assert ec.check_gradients_unimposed(lib, B=512, T=194, bound=3e-2, kind="graph_mixednet", flags=ec.GRAPH_MIXEDNET_FULL) <= 3e-2


def test_bf16_storage_mode_at_the_baseline_batch_4096(lib):
    """BASELINE configs[4] names batch 4096: forward parity and one train step of the bf16-storage mode at that size
    (the oracle rounds the same stored tensors)."""
    ec.check_forward_parity(lib, B=4096, T=194, training=True, flags=ec.BF16_STORED, lowp_tap_tol=1e-2)
    ec.check_train_steps(lib, B=4096, T=194, steps=1, grid=0, flags=ec.BF16_STORED)


@pytest.mark.parametrize("wide", [0, 1])
def test_block_backward_kernel_forms(lib, wide):
    """Every form of the block backward kernels, whichever is the library's default ("bwd_wide" 0 = 256 threads per 64-row
    tile: bwd_block_kernel; 1 = 512: bwd_blockw_kernel, kernels_bwdw.hip.h): ragged tiles, several windows per workgroup,
    graph replay, then the BASELINE configs[1] size against the float64 oracle with and without the engine's ReLU decisions."""
    flags = dict(ec.DEF, bwd_wide=wide)
    ec.check_train_steps(lib, B=6, T=194, steps=2, grid=0, flags=flags)
    ec.check_train_steps(lib, B=5, T=130, steps=1, grid=3, flags=flags)
    ec.check_train_steps(lib, B=64, T=194, steps=1, grid=16, graphs=True, flags=flags)
    worst = ec.check_train_steps(lib, B=1024, T=194, steps=1, grid=0, flags=flags)
    assert worst["l2_max"] <= 1e-4
    assert ec.check_gradients_unimposed(lib, B=1024, T=194, bound=1e-2, flags=flags) <= 1e-2


@pytest.mark.parametrize("wide", [0, 1])
def test_block_backward_kernel_forms_64_wide(lib, wide):
    flags = dict(ec.NOTEBOOK, bwd_wide=wide)
    ec.check_train_steps(lib, B=9, T=231, steps=1, grid=8, flags=flags)
    worst = ec.check_train_steps(lib, B=600, T=204, steps=1, grid=0, flags=flags)
    assert worst["l2_max"] <= 1e-4
    assert ec.check_gradients_unimposed(lib, B=512, T=204, bound=2e-2, flags=dict(ec.CROSSED[4], bwd_wide=wide)) <= 2e-2


@pytest.mark.parametrize("wide", [0, 1])
def test_determinism_of_the_block_backward_forms(lib, wide):
    outs = []
    for _ in range(2):
        om = ec.perturbed_oracle(194)
        lay, eng = ec.make_engine(lib, 194, 700, om, flags=dict(ec.DEF, bwd_wide=wide))
        rng = np.random.default_rng(5)
        eng.set_batch(ec.synth_x(rng, 700, 194))
        eng.set_targets((rng.random(700) < 0.5).astype(np.float32), np.ones(700, np.float32))
        eng.train_step(700, 1e-3)
        outs.append(eng.get_grads())
        eng.close()
    np.testing.assert_array_equal(outs[0], outs[1])


WIDER_TABLE = [dict(ec.DEF, pointwise_filters="32,32,32,32", mixconv_kernel_sizes="[3],[7],[17],[19]"),
               dict(ec.DEF, pointwise_filters="32,48,64,48", mixconv_kernel_sizes="[7],[5,9],[3],[11,15]", first_conv_kernel_size=5, stride=2),
               dict(ec.DEF, pointwise_filters="64,32,32,48,48", mixconv_kernel_sizes="[3],[5],[7],[9],[23]", repeat_in_block="1,1,1,1,1",
                    residual_connection="0,0,0,0,0"),
               dict(ec.DEF, pointwise_filters="48,64,64,32", mixconv_kernel_sizes="[5],[19],[21],[3]", stride=3, first_conv_kernel_size=3)]


@pytest.mark.parametrize("which", range(len(WIDER_TABLE)))
def test_block_kernels_of_the_wider_shape_table(lib, which):
    """Shapes the round-5 table added (csrc/block_launch.hip.h): 32-wide and mixed-width blocks, kernel lengths 3 / 7 / 17 / 19 /
    23, stride-2 / stride-3 first convolutions, five blocks (a strided first convolution WITH a 3-tap depthwise behind it, in
    tail mode: test_first_block_tail_k_step_with_a_three_tap_depthwise) - on the specialised block kernels
    (asserted), forward parity, a train step with ragged tiles and several windows per workgroup, and at B = 256 without imposed
    ReLU decisions."""
    from microwakeword_amd import mixednet
    flags = WIDER_TABLE[which]
    T = 230
    assert mixednet.kernel_family(flags, T, lib=lib)[0] == "block"
    ec.check_forward_parity(lib, B=5, T=T, training=True, grid=3, flags=flags)
    ec.check_train_steps(lib, B=37, T=T, steps=1, grid=16, flags=flags)
    assert ec.check_gradients_unimposed(lib, B=256, T=T, bound=2e-2, flags=flags) <= 2e-2


@pytest.mark.parametrize("wide", [0, 1])
def test_first_block_tail_k_step_with_a_three_tap_depthwise(lib, wide):
    """Tail-mode lengths (Ta in {65, 66}) of a strided first convolution with a 3-tap depthwise behind it (TAIL = 2 < the four
    rows of the tail k-step), both forms of the first-block backward - the case the wider-table test above never reaches
    (T = 230 is not in tail mode, and its [3] cases have stride 1)."""
    for stride, lengths in ((3, (195, 197, 200)), (2, (131, 134))):
        flags = dict(ec.DEF, mixconv_kernel_sizes="[3],[9],[13],[21]", stride=stride, bwd_wide=wide)
        for T in lengths:
            ec.check_train_steps(lib, B=37, T=T, steps=1, grid=16, flags=flags)
    # a 5- / 7-tap first depthwise: TAIL = 4 / 6 tail rows = one / TWO tail k-steps (round-6 fuzz finding: the second was missing)
    for k, stride, lengths in ((7, 3, (207, 209, 212)), (7, 2, (139, 141)), (5, 3, (204, 206))):
        flags = dict(ec.DEF, mixconv_kernel_sizes="[%d],[9],[13],[21]" % k, stride=stride, bwd_wide=wide)
        for T in lengths:
            ec.check_train_steps(lib, B=37, T=T, steps=1, grid=16, flags=flags)


def test_conv1_x6_against_the_exact_fp32_form(lib):
    """Round 6: the first convolution and its weight gradient as six bf16 slice products per fp32 product (the default for
    stride-1 first convolutions; ds_read_b64_tr_b16 operands in the backward kernel) against the exact-fp32 MFMA form of the
    same kernels (option "conv1_x6" 0): probabilities within 2e-6, gradients within 5e-6 per tensor when no ReLU decision
    differs between the forms (every call reads both forms' decisions; engine_checks says what a flip costs), not bit-identical
    (the option is wired); each form against the float64 oracle with its own ReLU decisions imposed.  Values over the whole uint16
    range too (three-slice x: against the other form and against the float64 oracle), and a 5-tap first conv."""
    small = ec.check_conv1_x6_against_the_f32_form(lib, B=12, T=194)
    assert small <= 5e-6, small          # (no flip in this batch on the device; the emulated kernels agree to 1.6e-6 here)
    for form in (0, 1):
        worst = ec.check_train_steps(lib, B=256, T=194, steps=1, grid=0, flags=dict(ec.DEF, conv1_x6=form, conv1_x6_fwd=form))
        assert worst["l2_max"] <= 1e-4
    ec.check_conv1_x6_against_the_f32_form(lib, B=256, T=194)
    ec.check_conv1_x6_against_the_f32_form(lib, B=37, T=111, raw_u16_range=True)
    # the x6 form against the float64 oracle itself on full-range uint16 inputs (x up to 2560: three significant slices)
    worst = ec.check_train_steps(lib, B=37, T=111, steps=1, grid=0, flags=dict(ec.DEF, conv1_x6=1, conv1_x6_fwd=1), raw_u16_range=True)
    assert worst["l2_max"] <= 1e-4
    ec.check_conv1_x6_against_the_f32_form(lib, B=64, T=150, flags=dict(ec.DEF, first_conv_kernel_size=5, pointwise_filters="32,48,64,48"))
    ec.check_conv1_x6_against_the_f32_form(lib, B=64, T=150, flags=dict(ec.DEF, pointwise_filters="64,64,64,64", mixconv_kernel_sizes="[7],[9],[13],[21]"))


def test_wide_first_block_backward_with_x6(lib):
    """Option "bwd_first_wide": the 512-thread form of the stride-1 first block's backward kernel with the conv1 weight gradient as
    bf16 slice products, against the float64 oracle (ragged tiles, several windows per workgroup, B = 1024 with imposed and without
    imposed ReLU decisions, 32 / 48 / 64 pointwise filters, run-to-run bit equality)."""
    for flags in (ec.DEF, dict(ec.DEF, pointwise_filters="32,48,48,48"), dict(ec.DEF, pointwise_filters="64,64,64,64", mixconv_kernel_sizes="[7],[9],[13],[21]")):
        ec.check_train_steps(lib, B=37, T=230, steps=1, grid=16, flags=dict(flags, bwd_first_wide=1))
    worst = ec.check_train_steps(lib, B=1024, T=194, steps=1, grid=0, flags=dict(ec.DEF, bwd_first_wide=1))
    assert worst["l2_max"] <= 1e-4
    assert ec.check_gradients_unimposed(lib, B=512, T=194, bound=2e-2, flags=dict(ec.DEF, bwd_first_wide=1)) <= 2e-2
    outs = []
    for _ in range(2):
        om = ec.perturbed_oracle(194)
        lay, eng = ec.make_engine(lib, 194, 300, om, flags=dict(ec.DEF, bwd_first_wide=1))
        rng = np.random.default_rng(5)
        eng.set_batch(ec.synth_x(rng, 300, 194))
        eng.set_targets((rng.random(300) < 0.5).astype(np.float32), np.ones(300, np.float32))
        eng.train_step(300, 1e-3)
        outs.append(eng.get_grads())
        eng.close()
    np.testing.assert_array_equal(outs[0], outs[1])


def test_reference_train_loop_trace_replay(lib, tmp_path):
    """what the reference's OWN train loop does with this package's objects.  In the build container
    ``oracle/ref_train_shim.py`` executes /root/reference/microwakeword/train.py unmodified against ``Model`` + ``FeatureHandler`` on the
    host-emulated library (tests/test_reference_train_loop.py) and records every call it makes on the two objects and what came
    back (tests/golden/ref_train_trace.json: 24 steps, two schedule phases, non-uniform class and penalty weights through the
    [B,B] matrix of train.py:288-293, three validation passes with the ambient split, weights + checkpoint writes).  Here the
    recorded call sequence is replayed on the MI355X (tests/ref_train_replay.py; /root/reference does not exist on this box): the
    five numbers train.py reads after every step and every ``evaluate`` result must come back as recorded, up to what float32
    rounding differences between the emulated and the real kernels grow to over 24 optimizer steps."""
    import ref_train_replay as rr
    fx = rr.load_fixture()
    worst, evals, cfg = rr.replay(fx, ec, lib, tmp_path)
    print("reference-loop replay: worst |difference| of (accuracy, recall, precision, auc, loss) over %d steps: %s" % (len(fx["steps"]), worst))
    assert worst[:3].max() <= 0.02 and worst[3] <= 0.01 and worst[4] <= 5e-3, worst
    for got, want in zip(evals, fx["evals"]):
        for k in ("accuracy", "recall", "precision", "auc"):
            assert abs(got[k] - want[k]) <= 0.02, (k, got[k], want[k])
        assert abs(got["loss"] - want["loss"]) <= 5e-3 * (1 + want["loss"]), (got["loss"], want["loss"])
        for k in ("tp", "fp", "tn", "fn"):   # (a window whose probability sits on one of the 101 cutoffs changes side with the last bits of the weights)
            assert np.abs(got[k] - np.array(want[k], np.float32)).max() <= 5, k
    for f in ("last_weights.weights.h5.npz", "best_weights.weights.h5.npz", "restore/ckpt.weights.npz", "restore/ckpt.opt.npz"):
        assert os.path.isfile(os.path.join(cfg["train_dir"], f)), f


def test_training_reduces_loss(lib):
    ec.check_training_reduces_loss(lib)


def test_determinism(lib):
    """Fixed-order partial sums: two identical steps give bit-identical gradients."""
    outs = []
    for _ in range(2):
        om = ec.perturbed_oracle(194)
        lay, eng = ec.make_engine(lib, 194, 32, om)
        rng = np.random.default_rng(5)
        eng.set_batch(ec.synth_x(rng, 32, 194))
        eng.set_targets((rng.random(32) < 0.5).astype(np.float32), np.ones(32, np.float32))
        eng.train_step(32, 1e-3)
        outs.append(eng.get_grads())
        eng.close()
    np.testing.assert_array_equal(outs[0], outs[1])


def test_notebook_topology_stride3_mixconv_groups(lib):
    """The topology the reference's notebook trains (first conv 5x1 stride 3, 64 filters, MixConv groups)."""
    ec.check_forward_parity(lib, B=4, T=204, training=False, flags=ec.NOTEBOOK)
    ec.check_forward_parity(lib, B=9, T=204, training=True, flags=ec.NOTEBOOK)
    ec.check_train_steps(lib, B=8, T=204, steps=2, grid=0, flags=ec.NOTEBOOK)
    ec.check_train_steps(lib, B=600, T=204, steps=1, grid=512, flags=ec.NOTEBOOK)   # grids above the topology's defaults


@pytest.mark.parametrize("training", [False, True])
def test_inception_forward(lib, training):
    """BASELINE config 4: default Inception (stem SSN(4), three 3-branch blocks), forward parity."""
    ec.check_inception_forward(lib, B=9, T=194, training=training)


def test_inception_forward_batch1024(lib):
    assert ec.check_inception_forward(lib, B=1024, T=194, training=False) <= ec.FWD_TOL


def test_inception_train_steps(lib):
    ec.check_inception_train_steps(lib, B=8, T=194, steps=3, grid=0)
    ec.check_inception_train_steps(lib, B=6, T=194, steps=2, grid=0, graphs=True)


def test_inception_variant_dilation_groups_two_stems(lib):
    ec.check_inception_forward(lib, B=5, T=120, training=True, flags=ec.INC_VARIANT)
    ec.check_inception_train_steps(lib, B=6, T=120, steps=2, grid=3, flags=ec.INC_VARIANT)


def test_graph_grid_options(lib):
    ec.check_graph_grid_options(lib, B=96, T=150)


def test_inception_generated_dropout(lib):
    ec.check_inception_generated_dropout(lib, B=16, T=194)


@pytest.mark.parametrize("tag", ["u16", "f32"])
def test_validation_on_device(lib, gold, tag):
    """validation forward + threshold metrics with the windows resident in HBM."""
    ec.check_validation_on_device(lib, gold, tag)


def _dp_world1_step(lib, library_comm, sync_bn, buckets):
    """One data-parallel train step in a world of one rank on the real device path, against the oracle."""
    import torch

    from microwakeword_amd.layout import MixedNetLayout
    from microwakeword_amd.parallel import DataParallel
    T, B = 194, 8
    device = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(stream):
        om = ec.perturbed_oracle(T)
        lay = MixedNetLayout(ec.DEF, T)
        eng = native.Engine(lib=lib, stream=stream.cuda_stream, **lay.engine_args(B))
        p, st = lay.pack(om.get_weights())
        eng.set_params(p)
        eng.set_bn_state(st)
        dp = DataParallel.for_engine(eng, device, sync_bn=sync_bn, grad_buckets=buckets, library_comm=library_comm)
        rng = np.random.default_rng(11)
        x = ec.synth_x(rng, B, T)
        y = (rng.random(B) < 0.5).astype(np.float32)
        w = np.ones(B, np.float32)
        eng.set_batch(x)
        eng.set_targets(y, w)
    # the step itself is issued OUTSIDE the torch stream context: the exchange must order itself against the engine's
    # stream, not against whatever stream happens to be current
    dp.train_step(B, 1e-3)
    pr, _, loss = eng.read_outputs(B)
    g = eng.get_grads()
    lo, po, grads, _ = om.loss_and_grads(x, y, w)
    gref = ec.oracle_grads_native_order(lay, om, grads)
    assert abs(loss - lo) <= 1e-5 * max(1.0, abs(lo))
    assert np.abs(pr - po).max() <= ec.FWD_TOL
    assert np.linalg.norm(g - gref) <= 2e-3 * np.linalg.norm(gref)
    om.train_step(x, y, w, 1e-3)
    p_ref, s_ref = lay.pack(om.get_weights())
    well = np.abs(gref) > 1e-4 * np.abs(gref).max()
    assert np.abs(eng.get_params() - p_ref)[well].max() <= 0.05 * 1e-3
    assert np.abs(eng.get_bn_state() - s_ref).max() <= 1e-5 * max(1.0, np.abs(s_ref).max())
    out = (eng.get_params().copy(), g.copy(), [f for _, f in dp.exchanges])
    eng.close()
    return out


def test_sync_bn_exchange_through_rccl_world1(lib):
    """The statistics / gradient exchange CALLBACK on the real device path: engine on a torch stream, RCCL
    process group of one rank, zero-copy views of the engine's HBM.  With W=1 the step must equal the
    plain one; what is exercised is the collapse -> all-reduce -> single-row finalize route, the hook
    trampoline and the stream ordering between the engine's kernels and the collectives."""
    import socket

    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        _, _, ex = _dp_world1_step(lib, library_comm=False, sync_bn=True, buckets=1)
        assert ex and all(f == native.EXCHANGE_IN_ORDER for f in ex)
        _, _, ex = _dp_world1_step(lib, library_comm=False, sync_bn=False, buckets=2)
        assert ex == [native.EXCHANGE_DEFERRED, native.EXCHANGE_IN_ORDER, native.EXCHANGE_FLUSH]
    finally:
        dist.destroy_process_group()


def test_exchange_through_the_library_s_own_rccl_communicator_world1(lib):
    """mww_allreduce_unique_id / mww_allreduce_init: ncclAllReduce issued by the library - on the engine's
    stream (in-order exchanges: sync-BN statistics, the one-bucket gradient) and on its own side stream ordered by events
    (the deferred first bucket of the two-bucket schedule).  One rank: the step equals the plain one, and the schedules
    equal each other bit for bit."""
    a = _dp_world1_step(lib, library_comm=True, sync_bn=False, buckets=1)
    b = _dp_world1_step(lib, library_comm=True, sync_bn=False, buckets=2)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    _dp_world1_step(lib, library_comm=True, sync_bn=True, buckets=1)


def test_train_loop_data_parallel_world1_rccl(lib, tmp_path):
    """microwakeword_amd.train.train as the single rank of an RCCL job: see engine_checks."""
    dp = ec.check_train_loop_data_parallel_world1(lib, tmp_path, "nccl")
    assert dp.library_comm


def test_bf16_pointwise_mode(lib):
    """BASELINE configs[4] "default mixednet bf16 with MFMA pointwise": forward and train step against the
    oracle that rounds the same operands to bf16; and within the 1e-3 forward tolerance of the fp32 oracle."""
    ec.check_forward_parity(lib, B=7, T=194, training=False, flags=ec.BF16)
    ec.check_forward_parity(lib, B=1024, T=194, training=True, flags=ec.BF16)
    ec.check_train_steps(lib, B=8, T=194, steps=2, grid=0, flags=ec.BF16)
    ec.check_train_steps(lib, B=6, T=204, steps=1, grid=0, flags=dict(ec.NOTEBOOK, pw_bf16=True))
    # against the plain fp32 oracle the bf16 mode stays inside the forward tolerance on this batch
    T, B = 194, 64
    om = ec.perturbed_oracle(T)
    lay, eng = ec.make_engine(lib, T, B, om, flags=ec.BF16)
    x = ec.synth_x(np.random.default_rng(3), B, T)
    eng.set_batch(x)
    eng.forward(B, training=False)
    pr, _, _ = eng.read_outputs(B, want_loss=False)
    assert np.abs(pr - om.predict(x)).max() <= 5e-3
    eng.close()


def test_inception_statistics_hand_over_matches_finalize_launches(lib):
    """conv/BN graph kernels: accumulator rows folded by the first consumer launch (no finalize launches) against the
    finalize-launch path, default and SubSpectralNormalization variant topology, eager and captured."""
    ec.check_inception_bn_inline_matches_finalize(lib, B=64, T=194, steps=3)
    ec.check_inception_bn_inline_matches_finalize(lib, B=9, T=150, steps=3, flags=ec.INC_VARIANT)
    ec.check_inception_bn_inline_matches_finalize(lib, B=6, T=194, steps=2, fuse_heads=False)


@pytest.mark.parametrize("which", range(5))
def test_crossed_topologies_on_the_block_kernels(lib, which):
    """Either documented width (48 / 64 filters) with either kernel set ([5],[9],[13],[21] / [5],[7,11],[9,15],[23]) and either
    first conv (3x1 / 5x1 stride 3 or 1) runs on the specialised block kernels: forward and train steps vs the oracle."""
    flags = ec.CROSSED[which]
    T = 204 if flags.get("stride", 1) == 3 else 194
    ec.check_forward_parity(lib, B=9, T=T, training=True, flags=flags)
    ec.check_train_steps(lib, B=8, T=T, steps=2, grid=0, flags=flags)
    ec.check_train_steps(lib, B=5, T=T - 37, steps=1, grid=3, flags=flags)


def test_bf16_storage_mode(lib):
    """BASELINE configs[4], full form ("storage_bf16"): the block outputs p_k and the stashed gradients g_k live in HBM
    as bf16 (fp32 accumulation, fp32 BN sums from the unrounded values), against the oracle that rounds the same stored
    tensors; the notebook topology (64 channels, stride 3) and the BASELINE batch size included."""
    ec.check_forward_parity(lib, B=7, T=194, training=False, flags=ec.BF16_STORED)
    ec.check_forward_parity(lib, B=1024, T=194, training=True, flags=ec.BF16_STORED)
    ec.check_train_steps(lib, B=8, T=194, steps=2, grid=0, flags=ec.BF16_STORED)
    ec.check_train_steps(lib, B=5, T=130, steps=1, grid=0, graphs=True, flags=ec.BF16_STORED)
    ec.check_train_steps(lib, B=6, T=204, steps=1, grid=0, flags=dict(ec.NOTEBOOK, st_bf16=True))
    # switching the option off again restores the exact fp32 path
    T, B = 194, 16
    om = ec.perturbed_oracle(T)
    lay, eng = ec.make_engine(lib, T, B, om, flags=ec.BF16_STORED)
    eng.set_option("pointwise_bf16", 0)
    x = ec.synth_x(np.random.default_rng(3), B, T)
    eng.set_batch(x)
    eng.forward(B, training=False)
    pr, _, _ = eng.read_outputs(B, want_loss=False)
    assert np.abs(pr - om.predict(x)).max() <= 1e-3
    eng.close()


@pytest.mark.parametrize("kind", ["mixednet", "inception"])
def test_train_loop_end_to_end(lib, tmp_path, kind):
    """The whole host loop (schedule, device-resident batches and validation, best-weights rule, checkpoint and
    restore) on a small separable task: the model has to learn it."""
    ec.check_train_loop_end_to_end(lib, tmp_path, B=32, steps=450, kind=kind, min_val_accuracy=0.95)


def test_mixednet_on_generic_graph_kernels(lib):
    """MixedNet flag combinations outside the specialised block kernels (repeat_in_block 2,
    a block without depthwise, odd filter counts, strided first conv, no first conv) on the graph kernels."""
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET, B=8, T=100, steps=2, grid=0)
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET, B=8, T=100, steps=1, grid=0, bn_inline=0)   # finalize launches instead of the hand-over
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET_NOCONV1, B=6, T=60, steps=2, grid=0, graphs=True)
    # the default topology through the generic route agrees with the oracle as well (cross-check of both kernel families)
    ec.check_graph_mixednet(lib, ec.DEF, B=4, T=194, steps=1, grid=0)


def test_mixednet_residual_connections(lib):
    """residual_connection: 1x1 conv + BN branch of the block input added before every repeat's ReLU (also in
    front of the classifier head)."""
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET_RESIDUAL, B=8, T=80, steps=2, grid=0)
    ec.check_graph_mixednet(lib, dict(ec.DEF, residual_connection="1,1,1,1"), B=5, T=194, steps=1, grid=0, graphs=True)


def test_mixednet_attention_and_pooled_heads(lib):
    """--spatial_attention / --pooled / --max_pool heads of MixedNet (mixednet.py:234-275,362-381)."""
    for flags in ec.GRAPH_MIXEDNET_HEADS:
        ec.check_graph_mixednet(lib, flags, B=6, T=64, steps=2, grid=0)
    ec.check_graph_mixednet(lib, dict(ec.DEF, spatial_attention=1, pooled=1), B=5, T=194, steps=1, grid=0, graphs=True)


@pytest.mark.parametrize("B,T", [(1, 47), (2, 48), (3, 300), (1023, 194), (257, 111)])
def test_edge_batch_sizes_and_lengths(lib, B, T):
    """Smallest spectrogram the default network accepts (one output frame), lengths off the tile grid, batch
    sizes that are neither powers of two nor multiples of the grid."""
    ec.check_forward_parity(lib, B=B, T=T, training=True)
    if B <= 3:
        ec.check_train_steps(lib, B=max(B, 2), T=T, steps=1, grid=0)


def test_long_run_stays_finite(lib):
    """2000 steps on a fixed random batch: loss, weights and BN state stay finite, and the batch is memorised."""
    from oracle import model_oracle as mo
    import torch
    om = mo.OracleModel("mixednet", ec.DEF, 194, seed=3, dtype=torch.float32)   # Keras default initialisation
    lay, eng = ec.make_engine(lib, 194, 64, om)
    eng.set_option("graphs", 1)
    rng = np.random.default_rng(0)
    x = ec.synth_x(rng, 64, 194)
    y = (rng.random(64) < 0.5).astype(np.float32)
    eng.set_batch(x)
    eng.set_targets(y, np.ones(64, np.float32))
    losses = []
    for s in range(2000):
        eng.train_step(64, 1e-3)
        if s % 400 == 399:
            losses.append(eng.read_outputs(64)[2])
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses   # it memorises the fixed batch
    assert np.all(np.isfinite(eng.get_params())) and np.all(np.isfinite(eng.get_bn_state()))
    eng.close()


def test_data_path_fuzz(lib):
    """Random feature sets / policies / truncation strategies: sampler + HIP assembly bit-exact against the oracle."""
    ec.check_data_fuzz(lib, cases=40)


def test_mixednet_topology_fuzz(lib):
    """Random MixedNet flag sets (widths, MixConv groups, repeats, residuals, strides, heads) on the graph kernels."""
    ec.check_topology_fuzz(lib, cases=16, B=5)


def test_full_size_properties_batch1024(lib):
    """Size-independent properties at BASELINE configs[1] size (B=1024, T=194), where the oracle is too slow to be the
    checker for the backward pass: (a) the gradient is exactly linear in a power-of-two scale of the sample weights,
    (b) the fused gradient-finish + Adam launch gives the same bits as the separate launches of the data-parallel
    route, (c) two runs give the same bits, (d) a permutation of the batch permutes the outputs and moves no
    statistic beyond rounding."""
    B, T = 1024, 194
    om = ec.perturbed_oracle(T)
    rng = np.random.default_rng(21)
    x = ec.synth_x(rng, B, T)
    y = (rng.random(B) < 0.3).astype(np.float32)
    w = rng.choice([0.5, 1.0, 1.5], size=B).astype(np.float32)

    def run(xb, yb, wb, flags=0, apply_after=False):
        lay, eng = ec.make_engine(lib, T, B, om)
        eng.set_batch(xb)
        eng.set_targets(yb, wb)
        eng.train_step(B, 1e-3, flags)
        if apply_after:
            eng.apply_gradients(1e-3, 1.0)
        out = dict(g=eng.get_grads(), p=eng.get_params(), s=eng.get_bn_state(), pr=eng.read_outputs(B)[0], loss=eng.read_outputs(B)[2])
        eng.close()
        return out

    a = run(x, y, w)
    b = run(x, y, 2.0 * w)
    np.testing.assert_array_equal(2.0 * a["g"], b["g"])                     # (a)
    assert b["loss"] == pytest.approx(2.0 * a["loss"], rel=1e-6)
    c = run(x, y, w, flags=native.STEP_NO_APPLY, apply_after=True)
    np.testing.assert_array_equal(a["g"], c["g"])                           # (b)
    np.testing.assert_array_equal(a["p"], c["p"])
    d = run(x, y, w)
    for k in ("g", "p", "s", "pr"):
        np.testing.assert_array_equal(a[k], d[k])                           # (c)
    perm = rng.permutation(B)
    e = run(x[perm], y[perm], w[perm])
    assert np.abs(e["pr"] - a["pr"][perm]).max() <= 1e-5                    # (d)
    assert np.abs(e["s"] - a["s"]).max() <= 1e-5 * max(1.0, np.abs(a["s"]).max())
    assert np.linalg.norm(e["g"] - a["g"]) <= 1e-4 * np.linalg.norm(a["g"])


def test_head_frames_beyond_the_widest_instantiation_are_refused_at_creation(lib):
    """64 channels x 390 final frames: refused when the model is created (not at the first forward); 384 frames - the widest head
    instantiation - train on the block kernels against the oracle."""
    ec.check_head_frame_limit_is_refused_at_creation(lib, B=3)
    ec.check_train_steps(lib, B=3, T=430, steps=1, grid=2, flags=dict(ec.DEF, pointwise_filters="48,48,48,64"))


def test_against_frozen_oracle_outputs(lib, golden_dir):
    """Committed fixture route: tests/golden/model_oracle_golden.npz."""
    ec.check_against_frozen_oracle(lib, golden_dir)


def test_against_the_reference_graph_fixture(lib, golden_dir):
    """tests/golden/ref_graph_golden.npz = the reference's own mixednet.py / inception.py executed over float64 stand-ins of the Keras
    layer primitives (oracle/ref_model_shim.py): probabilities, loss, every gradient, BN moving statistics."""
    print(ec.check_against_reference_graph_fixture(lib, golden_dir))


def test_frame_chunks_of_the_pointwise_graph_ops(lib):
    """"graph_frame_chunks" on the GPU (round 2 shipped these kernels emulator-tested only): the 1x1 ops of a conv/BN graph
    process a window as 2-4 frame chunks - Inception and MixedNet graphs, uneven last chunks, the automatic setting, a captured
    graph - against the oracle; and every setting gives the same parameters as whole windows up to fp32 summation order."""
    ec.check_inception_train_steps(lib, B=6, T=121, steps=2, grid=2, options={"graph_frame_chunks": 2})
    ec.check_inception_train_steps(lib, B=5, T=120, steps=1, grid=0, options={"graph_frame_chunks": 3})
    ec.check_inception_train_steps(lib, B=4, T=194, steps=1, grid=0, options={"graph_frame_chunks": 1})
    ec.check_inception_train_steps(lib, B=6, T=120, steps=1, grid=2, flags=ec.INC_VARIANT, options={"graph_frame_chunks": 4})
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET, B=8, T=100, steps=2, grid=0, options={"graph_frame_chunks": 3})
    ec.check_graph_mixednet(lib, ec.GRAPH_MIXEDNET_NOCONV1, B=4, T=60, steps=1, grid=1, graphs=True, options={"graph_frame_chunks": 2})
    ec.check_graph_mixednet(lib, ec.DEF, B=64, T=194, steps=1, grid=0, options={"graph_frame_chunks": 0})   # the non-default setting for such graphs


def test_tf_golden_vectors(lib, tmp_path):
    """The engine against the reference's own TensorFlow numbers (tests/golden/tf_golden.npz, tools/make_tf_golden.py) when the
    file exists; always against a file of the same schema synthesized from the oracle, so the consumer stays exercised."""
    import os

    import tf_golden as tg
    z = np.load(tg.synthesize(str(tmp_path / "tf_like.npz"), cases=("mixednet_default", "inception_default")))
    for case in z["cases"]:
        tg.check_engine(lib, z, str(case))
    if os.path.isfile(tg.GOLDEN):
        z = np.load(tg.GOLDEN)
        for case in z["cases"]:
            tg.check_engine(lib, z, str(case))


def test_prefetched_batches_train_like_the_synchronous_sampler(lib):
    ec.check_prefetched_training_matches_synchronous(lib, B=64, T=194, steps=7)


def test_train_loop_prefetch_is_schedule_only(lib, tmp_path):
    ec.check_train_loop_prefetch_is_schedule_only(lib, tmp_path)


def test_first_conv_tail_rows(lib):
    ec.check_first_conv_tail_rows(lib, B=37, grid=0)


def test_inception_static_shapes_are_schedule_only(lib):
    ec.check_inception_static_shapes_are_schedule_only(lib, B=67, lengths=(100, 194, 208, 212, 236))


def test_bn_inline_matches_finalize(lib):
    ec.check_bn_inline_matches_finalize(lib, B=96, T=194, steps=4)
    ec.check_bn_inline_matches_finalize(lib, B=5, T=194, steps=2)   # fewer workgroups than accumulator rows
    ec.check_bn_inline_matches_finalize(lib, B=1024, T=194, steps=3)
    ec.check_bn_inline_matches_finalize(lib, B=33, T=204, steps=3, flags=ec.NOTEBOOK)


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_fused_input_is_bit_identical(lib, dtype):
    ec.check_fused_input(lib, B=64, T=194, steps=4, dtype=dtype)
    ec.check_fused_input(lib, B=5, T=100, steps=3, dtype=dtype)


def test_fused_input_through_captured_graphs(lib):
    ec.check_fused_input(lib, B=64, T=194, steps=20, graphs=True)


def test_gather_fuzz(lib):
    ec.check_gather_fuzz(lib, cases=150)
    ec.check_gather_fuzz(lib, cases=20, first=200, notebook=True)


def test_inception_topology_fuzz(lib):
    """Random Inception flag sets (stem layers, blocks, kernel sizes, dilation, sub-spectral groups, dropout).  Found the
    twin-launch race of unfused branch heads that share a producer (fixed in mww_create_convnet's twin rule)."""
    ec.check_inception_topology_fuzz(lib, cases=60)


def test_shape_fuzz(lib):
    """12 of the random (frames, batch, grid) cases; tools/gpu_shape_fuzz.py ran 400 of them green."""
    ec.check_shape_fuzz(lib, cases=12, first=40)


def test_inception_stem_gathers_descriptor_only_batches(lib):
    ec.check_inception_gathered_stem(lib, cases=4, B=64, graphs=(0, 1))
    # the bench shape, two and four windows per workgroup (a fixed grid: the gathering kernels' own occupancy may give them
    # another number of partial rows than the dense ones - same gradient up to float32 summation order, not bit for bit)
    ec.check_inception_gathered_stem(lib, cases=1, first=4, B=1024, grid=512)
    ec.check_inception_gathered_stem(lib, cases=1, first=5, B=1024, grid=256)
    ec.check_inception_gathered_stem(lib, cases=1, first=6, B=40, grid=4)               # ten windows per workgroup: x is written out
    ec.check_inception_gathered_stem(lib, cases=1, first=7, B=40, grid=8, graphs=(1,))  # five per workgroup

