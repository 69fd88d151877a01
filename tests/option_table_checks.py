"""mww_set_option as one table (csrc/mww_lib.hip kOptions), shared by tests/test_option_table_emulated.py and its GPU twin:
every documented name is accepted on both kinds of context, ranges and refusals report the texts they always did, an
option of the other engine changes nothing, and a captured step is not replayed across an option change.  The contexts:
the default MixedNet on the block kernels and a two-block MixedNet flag set on the conv/BN graph engine, T = 60,
max_batch 2.  Every comparison is exact (``np.array_equal``): both sides run the same kernels on the same inputs."""
import os
import re

import numpy as np
import pytest

import engine_checks as ec
from microwakeword_amd import native
from microwakeword_amd.layout import GraphMixedNetLayout, MixedNetLayout

KINDS = ("mixednet", "graph")
T, B = 60, 2
# name -> default value (include/mww.h; csrc/engine.hip.h, block_engine.hip, graph_engine.hip)
DEFAULTS = {
    "graphs": 0, "grid_fwd": None, "grid_bwd": None, "grid_head": None, "grid_graph": 0, "dropout_seed": 0x5EED, "pointwise_bf16": 0,
    "storage_bf16": 0, "fused_input": 1, "bn_inline": 1, "tail_roles": 1, "bce_from_logits": 1, "graph_role_split": 1,
    "graph_dgrad_share": 50, "graph_fwd_wg_per_cu": 4, "graph_bwd_wg_per_cu": 4, "graph_frame_chunks": None, "graph_static_shapes": 1,
    "graph_planar": 1, "bwd_wide": 1, "conv1_x6": 1, "conv1_x6_fwd": 0, "bwd_first_wide": 0, "dp_commit_late": -1, "grad_buckets": 1,
    "assemble_split": 2, "side_stream": 0, "profile": 0, "profile_split": 0, "ablate": 0,
}
# name -> (a value below the range, one above it, the message); n_cu-relative upper bounds are passed far (1 << 30)
RANGES = {
    "graph_fwd_wg_per_cu": (0, 9, "graph_fwd_wg_per_cu must be 1..8"),
    "graph_bwd_wg_per_cu": (0, 9, "graph_bwd_wg_per_cu must be 1..8"),
    "graph_frame_chunks": (-1, 5, "graph_frame_chunks must be 0..4"),
    "graph_dgrad_share": (9, 91, "graph_dgrad_share must be 10..90"),
    "grad_buckets": (0, 3, "grad_buckets must be 1 or 2"),
    "assemble_split": (0, 9, "assemble_split out of range"),
    "dp_commit_late": (-2, 2, "dp_commit_late must be -1 (per-family defaults), 0 or 1"),
    "grid_fwd": (0, 1 << 30, "grid_fwd out of range"),
    "grid_bwd": (0, 1 << 30, "grid_bwd out of range"),
    "grid_graph": (-1, 1 << 30, "grid_graph out of range"),
    "grid_head": (0, 1 << 30, "grid_head out of range"),
}
# options of one engine that a context of the other kind accepts and ignores (a value away from the default)
GRAPH_ONLY = {"graph_role_split": 0, "graph_static_shapes": 0, "graph_planar": 0, "graph_fwd_wg_per_cu": 2, "graph_bwd_wg_per_cu": 2,
              "graph_frame_chunks": 2, "graph_dgrad_share": 30, "profile_split": 1, "grid_graph": 3, "dropout_seed": 7}
BLOCK_ONLY = {"ablate": 1, "bwd_wide": 0, "conv1_x6": 0, "conv1_x6_fwd": 1, "bwd_first_wide": 1, "dp_commit_late": 0, "grid_fwd": 1,
              "grid_bwd": 1, "pointwise_bf16": 0, "storage_bf16": 0}
GRAPH_FLAGS = ec.GRAPH_MIXEDNET_NOCONV1   # two blocks, convolutions + BatchNorm and depthwise ops: the statistics hand-over applies


def documented_names():
    """the quoted names of the option comment in front of mww_set_option"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mww.h")).read()
    comment = text[text.index('/* options: "graphs"'):text.index("int mww_set_option(")]
    return sorted(set(re.findall(r'"([a-z0-9_]+)"', comment)))


def engine(lib, kind):
    lay = MixedNetLayout(ec.DEF, T) if kind == "mixednet" else GraphMixedNetLayout(GRAPH_FLAGS, T)
    eng = native.Engine(lib=lib, **lay.engine_args(B))
    eng.set_grad_mask(lay.grad_mask())
    eng.set_params(np.random.default_rng(3).normal(0.0, 0.25, eng.n_params).astype(np.float32))
    return eng


def refusal(eng, name, value):
    with pytest.raises(native.NativeError) as e:
        eng.set_option(name, value)
    return str(e.value)


def check_documented_names_at_their_defaults(lib, kind):
    names = documented_names()
    assert set(names) == set(DEFAULTS), sorted(set(names) ^ set(DEFAULTS))
    eng = engine(lib, kind)
    for name in names:
        value = DEFAULTS[name]
        if value is None:   # depends on the device / the topology: a value every context accepts
            value = 0 if name == "graph_frame_chunks" else 1
        eng.set_option(name, value)
    eng.close()


def check_ranges_and_unknown_names(lib, kind):
    eng = engine(lib, kind)
    for name, (below, above, message) in RANGES.items():
        for value in (below, above):
            assert message in refusal(eng, name, value), (name, value)
    assert "unknown option: no_such_option" in refusal(eng, "no_such_option", 1)
    eng.close()


def check_bf16_is_refused_on_a_graph_context(lib):
    eng = engine(lib, "graph")
    for name in ("pointwise_bf16", "storage_bf16"):
        assert "the conv/BN graph kernels have no bf16 mode" in refusal(eng, name, 1)
        eng.set_option(name, 0)
    eng.close()


def _two_steps(lib, kind, options=(), graphs=0, between=()):
    eng = engine(lib, kind)
    for name, value in dict(options).items():
        eng.set_option(name, value)
    eng.set_option("graphs", graphs)
    rng = np.random.default_rng(17)
    for step in range(2):
        eng.set_batch(ec.synth_x(rng, B, T))
        eng.set_targets((rng.random(B) < 0.5).astype(np.float32), np.ones(B, np.float32))
        eng.train_step(B, 1e-2)
        if step == 0:
            for name, value in dict(between).items():
                eng.set_option(name, value)
    out = eng.get_params().copy(), eng.get_bn_state().copy(), eng.get_grads().copy()
    eng.close()
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def check_options_of_the_other_engine_change_nothing(lib, kind):
    plain = _two_steps(lib, kind)
    other = _two_steps(lib, kind, options=GRAPH_ONLY if kind == "mixednet" else BLOCK_ONLY)
    for a, b in zip(plain, other):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_replay_is_separated_by_an_option_change(lib):
    """graphs = 1: a step, "graph_dgrad_share" changed, a step == the same sequence without capture"""
    eager = _two_steps(lib, "graph", graphs=0, between={"graph_dgrad_share": 30})
    replay = _two_steps(lib, "graph", graphs=1, between={"graph_dgrad_share": 30})
    for a, b in zip(eager, replay):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
