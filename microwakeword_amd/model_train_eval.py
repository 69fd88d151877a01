"""CLI / config surface of the reference kept for the training path:
``python -m microwakeword_amd.model_train_eval --training_config cfg.yaml mixednet --residual_connection "0,0,0,0"``

Mirrors microwakeword/model_train_eval.py:
  * ``load_config(flags, model_module)``     :45-96   (YAML keys + derived ``summaries_dir, stride,
    spectrogram_length_final_layer, spectrogram_length, flags, training_input_shape``)
  * ``train_model(config, model, data_processor, restore_checkpoint)``   :99-128
  * ``evaluate_model``                         :131-272 (``--test_tf_nonstreaming``, ``--test_tflite_nonstreaming``,
    ``--test_tflite_streaming`` run natively through streaming.py, after ``--train 1`` or on an existing ``train_dir``; what
    a requested evaluation does not cover - stream-mode spatial attention, int8 with attention models, int8 with residual /
    pooled models unless ``--quantized_backend native_ext`` - raises before training starts)
  * argparse surface                          :277-389

Data-parallel over the GPUs of one node (no reference equivalent): launched as
``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m
microwakeword_amd.model_train_eval --training_config cfg.yaml mixednet ...`` every process reads ``RANK`` / ``LOCAL_RANK`` /
``WORLD_SIZE``, takes GPU ``LOCAL_RANK``, joins an RCCL process group and ``train.train`` does the rest (sharded providers,
gradient all-reduce inside the step, sharded validation, rank 0 writes the files).  ``batch_size`` of the YAML stays the
global batch.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

import yaml

from . import inception
from . import mixednet
from . import native
from .data import FeatureHandler
from . import train as train_mod


def get_input_data_shape(config):
    """layers/modes.py:40-64 for the TRAINING / NON_STREAM_INFERENCE modes."""
    return (config["spectrogram_length"], 40)


def load_config(flags, model_module):
    config = yaml.load(open(flags.training_config, "r").read(), yaml.Loader)
    config["summaries_dir"] = os.path.join(config["train_dir"], "logs/")
    config["stride"] = flags.__dict__.get("stride", 1)
    config["window_step_ms"] = config.get("window_step_ms", 20)
    sample_rate, window_size_ms = 16000, 30
    desired_samples = int(sample_rate * config["clip_duration_ms"] / 1000)
    window_size_samples = int(sample_rate * window_size_ms / 1000)
    window_step_samples = int(config["stride"] * sample_rate * config["window_step_ms"] / 1000)
    length_minus_window = desired_samples - window_size_samples
    if length_minus_window < 0:
        config["spectrogram_length_final_layer"] = 0
    else:
        config["spectrogram_length_final_layer"] = 1 + int(length_minus_window / window_step_samples)
    config["spectrogram_length"] = config["spectrogram_length_final_layer"] + model_module.spectrogram_slices_dropped(flags)
    config["flags"] = flags.__dict__
    config["training_input_shape"] = get_input_data_shape(config)
    return config


def save_model_summary(model, path, file_name="model_summary.txt"):
    """utils.py:131-145."""
    with open(os.path.join(path, file_name), "wt") as fd:
        model.summary(print_fn=lambda x: fd.write(x + "\n"))


def claim_train_dir(config, restore_checkpoint):
    """model_train_eval.py:99-120: the run owns a fresh ``train_dir`` unless it restores a checkpoint.  In a data-parallel
    job rank 0 creates the directory and every rank learns the outcome (one object broadcast), so that all of them raise
    - or none."""
    rank, world = train_mod.process_group()
    exists = False
    if rank == 0:
        try:
            os.makedirs(config["train_dir"])
            os.mkdir(config["summaries_dir"])
        except OSError:
            exists = True
    if world > 1:
        import torch.distributed as dist
        box = [exists]
        dist.broadcast_object_list(box, src=0)
        exists = box[0]
    if exists and not restore_checkpoint:
        raise ValueError("model already exists in folder %s" % config["train_dir"]) from None


def train_model(config, model, data_processor, restore_checkpoint):
    """model_train_eval.py:99-128: claims ``train_dir`` (a fresh directory, or an existing one only with
    ``restore_checkpoint``: "model already exists" otherwise), writes the configuration and the model summary, trains.
    Called once the model and the data processor exist - as in the reference - so a set-up failure leaves no directory."""
    claim_train_dir(config, restore_checkpoint)
    if train_mod.process_group()[0] == 0:
        with open(os.path.join(config["train_dir"], "training_config.yaml"), "w") as outfile:
            yaml.dump({k: v for k, v in config.items() if k != "features" or all("stores" not in f for f in v)}, outfile,
                      default_flow_style=False)
        save_model_summary(model, config["train_dir"])
    return train_mod.train(model, config, data_processor)


def init_process_group_from_env():
    """One process per GPU: ``RANK`` / ``LOCAL_RANK`` / ``WORLD_SIZE`` / ``MASTER_ADDR`` / ``MASTER_PORT`` as
    ``torch.distributed.run`` exports them.  Returns (rank, local_rank, world); (0, None, 1) outside such a launch - torch is
    not imported then.  The backend is RCCL (``"nccl"``); ``MWW_DIST_BACKEND=gloo`` serves host-emulated builds of the
    library (tests)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, None, 1
    import torch
    import torch.distributed as dist
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    backend = os.environ.get("MWW_DIST_BACKEND", "nccl")
    if not dist.is_initialized():
        if backend == "nccl":
            # 88 KB of gradient per step: latency-bound, one or two channels move it as fast as many
            os.environ.setdefault("NCCL_MAX_NCHANNELS", "2")
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local_rank, world


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--training_config", type=str, default="trained_models/model/training_parameters.yaml")
    parser.add_argument("--train", type=int, default=1)
    parser.add_argument("--test_tf_nonstreaming", type=int, default=0)
    parser.add_argument("--test_tflite_nonstreaming", type=int, default=0)
    parser.add_argument("--test_tflite_nonstreaming_quantized", type=int, default=0)
    parser.add_argument("--test_tflite_streaming", type=int, default=0)
    parser.add_argument("--test_tflite_streaming_quantized", type=int, default=0)
    parser.add_argument("--quantized_backend", type=str, default="tflite", choices=("tflite", "native", "native_ext"),
                        help="native: run --test_tflite_streaming_quantized on the int8 kernel here, calibrated and quantized "
                             "by a restatement of TFLite's int8 arithmetic (not TFLite itself); native_ext: native, plus the "
                             "restated int8 ADD / AVERAGE_POOL_2D / MAX_POOL_2D of MixedNets with --residual_connection or --pooled")
    parser.add_argument("--detections_cutoff", type=float, default=None,
                        help="with a --test_tflite_* evaluation that runs here: also write detections.txt / detections.npz next to "
                             "tflite_streaming_roc.txt - every ambient false accept (track, time, moving average) and every missed "
                             "positive at this probability cutoff")
    parser.add_argument("--operating_point_faph", type=float, default=None,
                        help="with a --test_tflite_* evaluation that runs here: also write operating_points.txt / operating_points.npz / "
                             "operating_point.json next to tflite_streaming_roc.txt - FAPH and FRR at every (sliding window, cutoff) "
                             "and the window and cutoff with the fewest false rejections at no more than this many false accepts per hour")
    parser.add_argument("--operating_point_windows", type=str, default=",".join(str(w) for w in range(1, 11)),
                        help="the sliding-window sizes of --operating_point_faph (comma separated, each 1..256, at most 32)")
    parser.add_argument("--operating_point_bootstrap", type=int, default=None,
                        help="with --operating_point_faph: also bootstrap the operating point on the device with this many replicates "
                             "(1..65536) and write operating_point_bootstrap.json (settings, percentile intervals of recall and FAPH at the "
                             "recommended point and of the recall re-selected per replicate) / operating_point_bootstrap.npz (one record per "
                             "replicate) next to operating_point.json")
    parser.add_argument("--operating_point_bootstrap_seed", type=int, default=0, help="seed of the bootstrap's counter hash (0 .. 2^64 - 1)")
    parser.add_argument("--operating_point_bootstrap_block", type=int, default=0,
                        help="ambient resampling unit in moving-average values: 0 resamples whole ambient tracks, a positive multiple of 1024 "
                             "blocks of that length")
    parser.add_argument("--operating_point_bootstrap_confidence", type=float, default=0.95, help="confidence of the percentile intervals (0 .. 1)")
    parser.add_argument("--restore_checkpoint", type=int, default=0)
    parser.add_argument("--use_weights", type=str, default="best_weights")
    parser.add_argument("--verbosity", type=str, default="INFO")
    parser.add_argument("--device", type=int, default=0, help="HIP device index (one process per GPU)")
    subparsers = parser.add_subparsers(dest="model_name", help="NN model name")
    inception.model_parameters(subparsers.add_parser("inception"))
    mixednet.model_parameters(subparsers.add_parser("mixednet"))
    return parser


def main(argv=None):
    parser = build_parser()
    flags, unparsed = parser.parse_known_args(argv)
    if unparsed:
        raise ValueError("Unknown argument: {}".format(unparsed))
    if flags.model_name == "mixednet":
        model_module = mixednet
    elif flags.model_name == "inception":
        model_module = inception
    else:
        raise ValueError("Unknown model type: {}".format(flags.model_name))
    already = "torch.distributed" in sys.modules and sys.modules["torch.distributed"].is_initialized()
    rank, local_rank, world = init_process_group_from_env()
    logging.basicConfig(level=getattr(logging, flags.verbosity.upper(), logging.INFO) if rank == 0 else logging.WARNING)
    try:
        return _run(flags, model_module, rank, local_rank, world)
    finally:
        if world > 1 and not already:   # the group this call created (a caller's own group is the caller's to end)
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


def evaluate_model(flags, model_module, config, device=0):
    """model_train_eval.py:131-272 ``evaluate_model`` on the MI355X: a fresh model loads ``<train_dir>/<use_weights>.weights.h5``
    (its ``.npz`` twin) and is evaluated on the test sets - ``--test_tf_nonstreaming``: ``non_stream/testing_set_metrics.txt``;
    ``--test_tflite_nonstreaming``: ``tflite_non_stream/tflite_streaming_roc.txt``; ``--test_tflite_streaming``:
    ``tflite_stream_state_internal/tflite_streaming_roc.txt`` (streaming.py); ``--test_tflite_streaming_quantized`` with
    ``--quantized_backend native`` or ``native_ext``: calibration and int8 quantization (quantize.py; Inception: quantize_graph.py;
    with ``native_ext`` a MixedNet with residual connections or a pooled head: quantize_mixednet.py), the parameters in
    ``tflite_stream_state_internal_quant/stream_state_internal_quant.npz`` and the ROC of the int8 streaming model in
    ``tflite_stream_state_internal_quant/tflite_streaming_roc.txt``.  No TFLite file is written: the streaming /
    non-streaming forms run natively from the same weights.  ``--operating_point_faph``: each of these ROC evaluations also
    writes the operating-point grid of ``streaming.operating_point_grid`` into its folder."""
    from . import streaming
    model = model_module.model(flags, config["training_input_shape"], config["batch_size"], device=device)
    model.load_weights(os.path.join(config["train_dir"], flags.use_weights + ".weights.h5"))
    data_processor = FeatureHandler(config, engine=model.engine)
    out = {}
    if flags.test_tf_nonstreaming:
        logging.info("Testing nonstreaming model")
        out["non_stream"] = streaming.model_accuracy(config, "non_stream", model, data_processor, data_set="testing",
                                                     accuracy_name="testing_set_metrics.txt")
    for flag, folder, mode in ((flags.test_tflite_nonstreaming, "tflite_non_stream", "non_stream"),
                               (flags.test_tflite_streaming, "tflite_stream_state_internal", "stream")):
        if flag:
            logging.info("Testing the %s model false accept per hour and false rejection rates at various cutoffs", mode)
            sm = streaming.StreamingModel(model, config["stride"], mode)
            out[folder] = streaming.streaming_model_roc(config, folder, sm, data_processor, data_set="testing",
                                                        ambient_set="testing_ambient", accuracy_name="tflite_streaming_roc.txt",
                                                        detections_cutoff=getattr(flags, "detections_cutoff", None))
            _operating_points(flags, config, folder, sm, data_processor)
    if getattr(flags, "test_tflite_streaming_quantized", 0):
        quantize = quantization_module(model, getattr(flags, "quantized_backend", "native"))
        folder = "tflite_stream_state_internal_quant"
        logging.info("Testing the quantized streaming model: calibrated and quantized by a restatement of TFLite's int8 "
                     "arithmetic (quantize.py / quantize_graph.py, INTEGRATION.md), not by TFLite")
        ranges = quantize.calibrate(model, data_processor, config)
        qm = quantize.quantize(model, ranges)
        path = os.path.join(config["train_dir"], folder)
        os.makedirs(path, exist_ok=True)
        qm.save(os.path.join(path, "stream_state_internal_quant.npz"))
        logging.info("int8 parameters:\n%s", qm.summary())
        qsm = streaming.QuantizedStreamingModel(qm, config["stride"], "stream", context=model)
        out[folder] = streaming.streaming_model_roc(config, folder, qsm, data_processor, data_set="testing",
                                                    ambient_set="testing_ambient", accuracy_name="tflite_streaming_roc.txt",
                                                    detections_cutoff=getattr(flags, "detections_cutoff", None))
        _operating_points(flags, config, folder, qsm, data_processor)
    return out


def operating_point_windows(flags):
    """The windows of ``--operating_point_faph`` (None without the flag), checked from the flags alone: ValueError for a target
    <= 0, a window outside 1..256, more than 32 windows, or no evaluation that runs here to attach the grid to."""
    target = getattr(flags, "operating_point_faph", None)
    if target is None:
        return None
    if not target > 0:
        raise ValueError("--operating_point_faph must be positive")
    try:
        windows = [int(w) for w in str(flags.operating_point_windows).split(",")]
    except ValueError:
        raise ValueError("--operating_point_windows must be comma-separated integers") from None
    if not 1 <= len(windows) <= native.OP_MAX_WINDOWS or any(not 1 <= w <= native.OP_MAX_WINDOW for w in windows):
        raise ValueError("--operating_point_windows takes 1..%d windows, each in 1..%d" % (native.OP_MAX_WINDOWS, native.OP_MAX_WINDOW))
    runs_here = getattr(flags, "test_tflite_streaming_quantized", 0) and getattr(flags, "quantized_backend", "tflite") in ("native", "native_ext")
    if not (flags.test_tflite_nonstreaming or flags.test_tflite_streaming or runs_here):
        raise ValueError("--operating_point_faph needs --test_tflite_nonstreaming, --test_tflite_streaming or a native "
                         "--test_tflite_streaming_quantized evaluation")
    return windows


def operating_point_bootstrap_settings(flags):
    """The ``bootstrap`` settings of ``--operating_point_bootstrap`` (None without the flag), checked from the flags alone:
    ValueError naming the flag for a value out of range, or without ``--operating_point_faph`` (any of the four flags)."""
    from . import streaming
    given = {name: getattr(flags, "operating_point_bootstrap" + ("_" + name if name != "replicates" else ""), default)
             for name, default in (("replicates", None),) + tuple((k, v) for k, v in streaming.BOOTSTRAP_DEFAULTS.items() if k != "replicates")}
    if given["replicates"] is None:
        if any(given[k] != v for k, v in streaming.BOOTSTRAP_DEFAULTS.items() if k != "replicates"):
            raise ValueError("--operating_point_bootstrap_seed / _block / _confidence need --operating_point_bootstrap")
        return None
    if getattr(flags, "operating_point_faph", None) is None:
        raise ValueError("--operating_point_bootstrap needs --operating_point_faph")
    try:
        return streaming.bootstrap_settings("--operating_point_bootstrap", given)
    except ValueError as e:
        raise ValueError(str(e).replace("--operating_point_bootstrap: bootstrap", "--operating_point_bootstrap (replicates) and its _seed / _block / "
                                        "_confidence flags")) from None


def _operating_points(flags, config, folder, sm, data_processor):
    """``--operating_point_faph``: the grid of the evaluation ``folder`` just ran, on the same tracks from the same start; with
    ``--operating_point_bootstrap`` also the bootstrap of its operating point, from the same start again"""
    windows = operating_point_windows(flags)
    if windows is None:
        return
    from . import streaming
    sm.reset()   # the ROC started from a fresh stream
    grid = streaming.operating_point_grid(config, folder, sm, data_processor, flags.operating_point_faph, windows, data_set="testing",
                                          ambient_set="testing_ambient")
    logging.info("%s: %s", folder, streaming.operating_point_text(grid).splitlines()[-1])
    boot = operating_point_bootstrap_settings(flags)
    if boot is not None:
        sm.reset()
        out = streaming.operating_point_bootstrap(config, folder, sm, data_processor, flags.operating_point_faph, windows, boot,
                                                  data_set="testing", ambient_set="testing_ambient")
        logging.info("%s: bootstrap intervals %s", folder, out["bootstrap"]["intervals"])


def quantization_module(model, backend="native"):
    """the module that calibrates and quantizes ``model``: the conversion does not depend on the family, the graph here does.
    ``native_ext`` sends a MixedNet whose flags ask for a residual connection or a pooled head to quantize_mixednet; for a plain
    MixedNet or an Inception model it is ``native``."""
    from . import quantize, quantize_graph, quantize_mixednet, streaming
    from .layout import InceptionLayout
    if isinstance(model.layout, InceptionLayout):
        return quantize_graph
    if backend == "native_ext" and streaming.mixednet_variant_flags(model.flags):
        return quantize_mixednet
    return quantize


def check_evaluation_flags(flags, model_module, config):
    """The topology check of the requested ``--test_*`` evaluations, from the flags alone: a MixedNet flag set one of them
    does not cover raises NotImplementedError here, not after the training run it would follow."""
    if model_module is not mixednet:
        return
    from . import streaming
    modes = [mode for flag, mode in ((flags.test_tflite_nonstreaming, "non_stream"), (flags.test_tflite_streaming, "stream")) if flag]
    int8 = bool(getattr(flags, "test_tflite_streaming_quantized", 0))
    if modes or int8:
        streaming.check_evaluation_topology(flags.__dict__, config["spectrogram_length"], config["stride"], modes, int8=int8,
                                            int8_variants=getattr(flags, "quantized_backend", "tflite") == "native_ext")


def check_mining_config(flags, model_module, config, world):
    """The ``hard_negative_mining`` mapping of the configuration (mining.mining_config) and the topology of the stream its
    rounds run on: a refusal is raised here, not at the first round of the training run."""
    from . import mining, streaming
    from .train import process_group
    m = mining.mining_config(config, max(int(world), process_group()[1]))
    if m is not None and model_module is mixednet:
        # quantized: the int8 family must cover the flag set (residual_connection and pooled are covered in the loop)
        streaming.check_evaluation_topology(flags.__dict__, config["spectrogram_length"], config["stride"], [m["mode"]],
                                            int8=bool(m.get("quantized")), int8_variants=True)
    return m


def check_streaming_validation_config(flags, model_module, config, world):
    """The ``streaming_validation`` mapping of the configuration (streaming.streaming_validation_config) and the topology of
    the stream it validates on: a refusal is raised here, not at the dry validation of the training run."""
    from . import streaming
    from .train import process_group
    v = streaming.streaming_validation_config(config, max(int(world), process_group()[1]))
    if v is not None and model_module is mixednet:
        streaming.check_evaluation_topology(flags.__dict__, config["spectrogram_length"], config["stride"], [v["mode"]],
                                            int8=bool(v.get("quantized")), int8_variants=True)
    return v


def _evaluate(flags, model_module, config, device, world):
    """rank 0 evaluates, the other ranks of a data-parallel job wait at a barrier"""
    if not any((flags.test_tf_nonstreaming, flags.test_tflite_nonstreaming, flags.test_tflite_streaming,
                getattr(flags, "test_tflite_streaming_quantized", 0))):
        return None
    from .train import process_group
    rank, world = process_group()
    out = evaluate_model(flags, model_module, config, device) if rank == 0 else None
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return out


def _run(flags, model_module, rank, local_rank, world):
    if flags.test_tflite_nonstreaming_quantized or (flags.test_tflite_streaming_quantized and flags.quantized_backend not in ("native", "native_ext")):
        msg = ("the int8 *_quantized evaluations need the TFLite converter's calibration (reference "
               "microwakeword.utils); --test_tf_nonstreaming, --test_tflite_nonstreaming and "
               "--test_tflite_streaming run here. --test_tflite_streaming_quantized also runs here with --quantized_backend "
               "native, on a restatement of TFLite's int8 arithmetic (not TFLite itself)")
        if flags.test_tflite_nonstreaming_quantized:
            msg += ("; --test_tflite_nonstreaming_quantized has no such restatement: the reference's calibration generator "
                    "yields stride-row chunks, which do not fit the non-streaming model's T-row input, so there is no "
                    "well-defined calibration to restate")
        raise NotImplementedError(msg)
    operating_point_windows(flags)
    operating_point_bootstrap_settings(flags)
    config = load_config(flags, model_module)
    check_evaluation_flags(flags, model_module, config)   # before training and before train_dir is claimed
    if flags.train:
        from .quantize import check_shared_calibration
        check_shared_calibration(check_mining_config(flags, model_module, config, world),   # likewise
                                 check_streaming_validation_config(flags, model_module, config, world))
        from . import qat
        qat.parse_config(config)   # weight_quantization_aware: likewise
        from . import averaging
        averaging.parse_config(config)   # weight_averaging: likewise
        from . import sharpness
        from .train import process_group
        sharpness.parse_config(config, max(int(world), process_group()[1]))   # sharpness_aware, gradient_clipping: likewise (single-device)
    device = flags.device if local_rank is None else local_rank
    if flags.train:
        device = flags.device if local_rank is None else local_rank
        if world > 1 and config["batch_size"] % world:
            raise ValueError("batch_size %d (the global batch) is not divisible by the %d ranks" % (config["batch_size"], world))
        # every rank's engine holds batch_size / W windows per step
        model = model_module.model(flags, config["training_input_shape"], config["batch_size"] // world, device=device)
        from .train import process_group
        rank, world = process_group()
        # a data-parallel rank uploads its shard of the training samples only (train() would shard an unsharded handler too)
        data_processor = FeatureHandler(config, engine=model.engine, shard=(rank, world) if world > 1 else None)
        if rank == 0:
            model.summary(print_fn=logging.getLogger("microwakeword_amd").info)
        result = train_model(config, model, data_processor, flags.restore_checkpoint)
        _evaluate(flags, model_module, config, device, world)
        return result
    if not os.path.isdir(config["train_dir"]):
        raise ValueError('model is not trained set "--train 1" and retrain it')
    return _evaluate(flags, model_module, config, device, world)


if __name__ == "__main__":
    main(sys.argv[1:])
