"""Throughput of the PRODUCT train loop (microwakeword_amd.train.train on the package's own Model / FeatureHandler) on the
synthetic benchmark stores, next to bench.py's figure for the same step: what a user of the CLI gets.
usage: python tools/train_loop_throughput.py [steps] [batch] [mixednet|inception] [streaming_validation] [quantized] [bootstrap]
With the fourth argument the configuration carries ``streaming_validation: {target_faph: 0.5}`` and the wall time of
the evaluation boundary is printed in its parts: validate_nonstreaming and each streaming validation (the dry one first).
With the fifth the session runs the loop twice, five boundaries each: with the float mapping, then with ``quantized: true``, whose
validation is printed in ITS parts too: LoopQuantizer.calibrate (mww_stream_calibrate over the 500 windows), quantize_weights (the
host quantization), QuantizedStreamingModel (the upload of the int8 parameters); the rest of validate_streaming is the run and
the summary.  With ``bootstrap`` as the last argument the mapping also carries ``bootstrap: {replicates: 1000}``: the
summary becomes ``operating_bootstrap``, inside validate_streaming."""
import random
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from microwakeword_amd import inception, mixednet, synthetic   # noqa: E402
from microwakeword_amd import train as tr   # noqa: E402
from microwakeword_amd.data import FeatureHandler   # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 600
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
kind = sys.argv[3] if len(sys.argv) > 3 else "mixednet"
with_streaming = len(sys.argv) > 4 and sys.argv[4] == "streaming_validation"
with_quantized = with_streaming and len(sys.argv) > 5 and sys.argv[5] == "quantized"
with_bootstrap = with_streaming and sys.argv[-1] == "bootstrap"
T = 194
timed = {}


def _timed(module, name, label=None):
    fn = getattr(module, name)

    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        timed.setdefault(label or name, []).append(time.perf_counter() - t0)
        return out
    setattr(module, name, wrapper)


from microwakeword_amd import quantize, streaming   # noqa: E402
_timed(tr, "validate_nonstreaming")
_timed(streaming, "validate_streaming")
if with_quantized:
    _timed(quantize.LoopQuantizer, "calibrate", "LoopQuantizer.calibrate")
    _timed(quantize, "quantize_weights")
    _timed(streaming.QuantizedStreamingModel, "__init__", "QuantizedStreamingModel")
for verbose in ((False, False) if with_quantized else (False, True)):
    cfg, _ = synthetic.benchmark_config(4096, 1234, n_val=256, n_ambient=32)
    d = tempfile.mkdtemp(prefix="mww_loop_")
    cfg = dict(cfg, train_dir=d, summaries_dir=d + "/logs", batch_size=B, spectrogram_length=T, training_steps=[steps], learning_rates=[1e-3],
               time_mask_max_size=[5], time_mask_count=[2], freq_mask_max_size=[5], freq_mask_count=[2], positive_class_weight=[1.0],
               negative_class_weight=[1.0], eval_step_interval=steps, target_minimization=0.9, minimization_metric=None,
               maximization_metric="accuracy")
    if with_streaming:
        cfg["streaming_validation"] = dict(target_faph=0.5, **(dict(bootstrap=dict(replicates=1000)) if with_bootstrap else {}))
    if with_quantized:
        cfg["eval_step_interval"] = max(1, steps // 5)
        cfg["streaming_validation"]["quantized"] = bool(timed)   # the second run of the session
        print("streaming_validation: %r" % (cfg["streaming_validation"],), flush=True)
    quantized_run = bool(with_quantized and timed)
    timed.clear()
    random.seed(0)
    np.random.seed(0)
    if kind == "inception":
        model = inception.model(dict(synthetic.DEFAULT_INCEPTION_FLAGS), (T, 40), B, seed=42, max_batch=B)
    else:
        model = mixednet.model(synthetic.DEFAULT_MIXEDNET_FLAGS, (T, 40), B, seed=42, max_batch=B)
    fh = FeatureHandler(cfg, engine=model.engine)
    t0 = time.perf_counter()
    tr.train(model, cfg, fh, verbose=verbose)
    dt = time.perf_counter() - t0
    sys.stdout.write("\n")
    print("train.train (%s) verbose=%s: %d steps of batch %d in %.3f s = %.4f ms/step = %.2f M windows/s (one validation pass and the "
          "checkpoint writes at the end included)" % (kind, verbose, steps, B, dt, 1e3 * dt / steps, steps * B / dt / 1e6), flush=True)
    print("evaluation boundary: " + "; ".join("%s %s ms" % (k, ", ".join("%.1f" % (1e3 * t) for t in v)) for k, v in timed.items()), flush=True)
    if quantized_run:
        parts = [timed[k] for k in ("LoopQuantizer.calibrate", "quantize_weights", "QuantizedStreamingModel")]
        rest = [v - sum(p[i] for p in parts) for i, v in enumerate(timed["validate_streaming"])]
        print("  of validate_streaming, run + summary (the rest): %s ms" % ", ".join("%.1f" % (1e3 * t) for t in rest), flush=True)
        med = lambda v: 1e3 * float(np.median(v[1:]))   # noqa: E731 - the dry validation creates the streams
        print("  medians after the dry validation: calibrate %.2f ms, host quantization %.2f ms, upload %.2f ms, run + summary %.2f ms, "
              "boundary %.2f ms; host quantization is %.0f %% of the boundary"
              % (med(parts[0]), med(parts[1]), med(parts[2]), med(rest), med(timed["validate_streaming"]),
                 100 * med(parts[1]) / med(timed["validate_streaming"])), flush=True)
    model.engine.close()
