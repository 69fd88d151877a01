"""Freezes what the REFERENCE'S OWN evaluation code computes into tests/golden/streaming_metrics_golden.npz (build container
only).

``microwakeword/test.py`` is executed unmodified with stand-in ``tensorflow`` / ``absl`` / ``microwakeword.inference`` modules in
``sys.modules``: the stand-in ``Model`` replays prescribed probability arrays (one per track), the stand-in feature handler
hands out track ids in place of spectrograms.  ``compute_false_accepts_per_hour``, ``generate_roc_curve`` and
``tflite_streaming_model_roc`` then run end to end on synthetic tracks with values on and next to the cutoffs, cooldown
collisions, short tracks, and both branches of ``generate_roc_curve`` (``faph[0] > 2`` and ``<= 2``).  The fixture holds the
probabilities, the derived false-accept counts, the FAPH, the FRR, the AUC and the exact file text.  The reference's sources
do not travel.

    python tests/golden/make_golden_streaming_metrics.py [--check]      # needs /root/reference
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "streaming_metrics_golden.npz")
REFERENCE = os.environ.get("MWW_REFERENCE", "/root/reference")


def synthetic_cases():
    """-> {case: (ambient probability arrays, testing probability arrays, testing labels)}, seeded"""
    rng = np.random.default_rng(2024)
    cases = {}
    # faph[0] > 2: busy ambient tracks; values on (float32 of k/100) and next to the cutoffs, bursts that collide with the cooldown
    amb = []
    for n in (400, 260, 5, 6, 1000):
        p = (rng.random(n) ** 3).astype(np.float32)
        on = rng.integers(0, n, size=max(1, n // 10))
        p[on] = np.float32(rng.integers(0, 101, size=on.size) / 100.0)
        nxt = rng.integers(0, n, size=max(1, n // 10))
        p[nxt] = np.nextafter(p[nxt], np.float32(rng.choice([0.0, 1.0])))
        if n > 100:
            p[50:90] = np.float32(0.93)       # one long burst: accepts every 25 values
            p[120:123] = np.float32(0.99)     # a short one inside the cooldown of nothing
        amb.append(np.clip(p, 0, 1).astype(np.float32))
    tst, lab = [], []
    for i in range(23):
        n = int(rng.integers(30, 140))
        p = (rng.random(n) ** 2).astype(np.float32)
        if i % 3 == 0:
            p[-10:] = np.float32(rng.integers(0, 101) / 100.0)
        tst.append(p)
        lab.append(i % 4 != 1)
    cases["busy"] = (amb, tst, lab)
    # faph[0] <= 2: long quiet ambient tracks (exact zeros never exceed cutoff 0), a handful of accepts
    amb = []
    for n in (400000, 300000):
        p = np.zeros(n, np.float32)
        p[1000:1010] = np.float32(0.8)
        p[90000:90003] = np.float32(0.55)
        amb.append(p)
    tst = [(rng.random(int(rng.integers(31, 120))) ** 0.5).astype(np.float32) for _ in range(12)]
    cases["quiet"] = (amb, tst, [True] * 12)
    return cases


def moving_average_lists():
    """direct inputs of compute_false_accepts_per_hour: moving averages incl. empty and shorter-than-window tracks"""
    rng = np.random.default_rng(77)
    out = [rng.random(int(n)).astype(np.float32) for n in (0, 3, 4, 40, 300)]
    out[3][5:30] = np.float32(0.51)
    return out


def run_reference():
    """executes the reference's test.py over the stand-ins; returns the fixture dict"""
    tf = types.ModuleType("tensorflow")
    absl = types.ModuleType("absl")
    absl_logging = types.ModuleType("absl.logging")
    absl_logging.info = lambda *a, **k: None
    absl.logging = absl_logging
    mww = types.ModuleType("microwakeword")
    mww.__path__ = []
    inference = types.ModuleType("microwakeword.inference")
    state = {}

    class Model:   # replays the probabilities of the track whose id the "spectrogram" carries
        def __init__(self, path, stride=1):
            self.stride = stride

        def predict_spectrogram(self, spectrogram):
            return [np.float32(v) for v in state["probs"][int(spectrogram[0])]]

    inference.Model = Model
    saved = {k: sys.modules.get(k) for k in ("tensorflow", "absl", "absl.logging", "microwakeword", "microwakeword.inference")}
    sys.modules.update({"tensorflow": tf, "absl": absl, "absl.logging": absl_logging, "microwakeword": mww,
                        "microwakeword.inference": inference})
    try:
        spec = importlib.util.spec_from_file_location("microwakeword.test", os.path.join(REFERENCE, "microwakeword", "test.py"))
        test = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(test)
        out = {}
        cutoffs = np.arange(0, 1.01, 0.01)
        mas = moving_average_lists()
        for i, ma in enumerate(mas):
            out["fa/ma%d" % i] = ma
        out["fa/n"] = np.int64(len(mas))
        out["fa/faph"] = np.asarray(test.compute_false_accepts_per_hour(mas, cutoffs, 25, stride=2, step_s=0.02), np.float64)
        for case, (amb, tst, lab) in synthetic_cases().items():
            n_amb = len(amb)
            state["probs"] = amb + tst

            class Handler:
                def get_data(self, mode, batch_size, features_length, truncation_strategy):
                    if mode == "testing_ambient":
                        return [np.array([i]) for i in range(n_amb)], np.zeros(n_amb), np.ones(n_amb)
                    return [np.array([n_amb + i]) for i in range(len(tst))], np.array(lab, bool), np.ones(len(tst))

            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, "f"))
                config = {"stride": 1, "window_step_ms": 20, "train_dir": d, "batch_size": 8, "spectrogram_length": 10}
                auc = test.tflite_streaming_model_roc(config, "f", Handler())
                with open(os.path.join(d, "f", "tflite_streaming_roc.txt")) as fh:
                    text = fh.read()
            # the intermediate values, from the reference's own functions on the same inputs
            from numpy.lib.stride_tricks import sliding_window_view
            amb_ma = [sliding_window_view(p, 5).mean(axis=-1) for p in amb]
            faph = test.compute_false_accepts_per_hour(amb_ma, cutoffs, 25, stride=1, step_s=0.02)
            hours = sum(len(m) * 1 * 0.02 / 3600.0 for m in amb_ma)
            counts = np.rint(faph * hours).astype(np.int64)
            pos = [p for p, l in zip(tst, lab) if l]
            scores = [np.max(sliding_window_view(p[25:], 5).mean(axis=-1)) for p in pos]
            frr = [1 - sum(i > c for i in scores) / len(scores) for c in cutoffs]
            x, y, c = test.generate_roc_curve(faph, frr, cutoffs)
            pos_tracks = amb + pos
            out.update({"%s/probs" % case: np.concatenate(pos_tracks).astype(np.float32),
                        "%s/offsets" % case: np.concatenate([[0], np.cumsum([len(p) for p in pos_tracks])]).astype(np.int64),
                        "%s/n_ambient" % case: np.int64(n_amb), "%s/counts" % case: counts, "%s/faph" % case: np.asarray(faph, np.float64),
                        "%s/frr" % case: np.asarray(frr, np.float64), "%s/x" % case: np.asarray(x, np.float64),
                        "%s/y" % case: np.asarray(y, np.float64), "%s/cut" % case: np.asarray(c, np.float64),
                        "%s/auc" % case: np.float64(auc), "%s/text" % case: np.array(text)})
        out["roc/probs"], out["roc/offsets"] = out["busy/probs"], out["busy/offsets"]
        out["roc/n_ambient"], out["roc/counts"] = out["busy/n_ambient"], out["busy/counts"]
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


if __name__ == "__main__":
    fx = run_reference()
    if "--check" in sys.argv:
        old = np.load(FIXTURE)
        bad = [k for k in fx if not np.array_equal(np.asarray(old[k]), np.asarray(fx[k]))]
        print("fixture matches" if not bad else "DIFFERS: %s" % bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(FIXTURE, **fx)
    print("wrote", FIXTURE, {k: np.asarray(v).shape for k, v in fx.items() if k.endswith(("auc", "counts"))})
