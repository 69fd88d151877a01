"""Generates tests/golden/live_data_golden.json by running the REFERENCE's own microwakeword/data.py (imported via
oracle/ref_data_shim.py) on the two cases tests/test_data_oracle.py holds the oracle to: the §8(d) synthetic benchmark
store, and the 40 random cases of engine_checks.random_data_case.  Run where the reference tree exists:
    python tests/golden/make_golden_live_data.py
Their batches are ~45 MB, so the fixture keeps a digest of every array (dtype, shape, sha256 of its bytes) and, for the
random cases, the first draw of both global RNG streams after the last batch; the oracle must reproduce all of it bit for
bit.  The inputs are seeded and rebuilt by the tests, so neither the reference tree nor this script is needed at test time."""
import hashlib
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

FIXTURE = os.path.join(HERE, "live_data_golden.json")
T = 194
POLICY = dict(freq_mix_prob=0.0, time_mask_max_size=5, time_mask_count=2, freq_mask_max_size=5, freq_mask_count=2)
FUZZ_CASES = 40


def digest(a, dtype=None):
    """-> {"dtype", "shape", "sha256"} of ``a`` (converted to ``dtype`` first when given: the reference's dtype)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def benchmark_stores():
    from oracle import data_oracle as do
    return do.synthetic_stores(64, 1234)


def reference_benchmark_store(ref):
    """Same seeds, same §8(d) synthetic store: one training batch of 64 from the reference's FeatureHandler."""
    from microwakeword_amd.ragged import write_ragged_store
    pos, neg = benchmark_stores()
    with tempfile.TemporaryDirectory() as tmp:
        write_ragged_store(os.path.join(tmp, "pos", "training", "a_mmap"), pos)
        write_ragged_store(os.path.join(tmp, "neg", "training", "a_mmap"), neg)
        config = {"stride": 1, "window_step_ms": 10, "features": [
            dict(type="mmap", features_dir=os.path.join(tmp, "pos"), truth=True, sampling_weight=2.0, penalty_weight=1.0, truncation_strategy="truncate_start"),
            dict(type="mmap", features_dir=os.path.join(tmp, "neg"), truth=False, sampling_weight=10.0, penalty_weight=1.0, truncation_strategy="random")]}
        random.seed(0)
        np.random.seed(0)
        fh = ref.FeatureHandler(config)
        return fh.get_data("training", 64, T, "default", POLICY)


def reference_fuzz_case(ref, case):
    """-> (two training batches, (random.random(), np.random.random()) drawn after them) from the reference."""
    import engine_checks as ec
    from microwakeword_amd.ragged import write_ragged_store
    Tc, provs, policy, B, strategy = ec.random_data_case(case)
    with tempfile.TemporaryDirectory() as tmp:
        feats = []
        for i, p in enumerate(provs):
            write_ragged_store(os.path.join(tmp, "p%d" % i, "training", "a_mmap"), p["store"])
            feats.append(dict(type="mmap", features_dir=os.path.join(tmp, "p%d" % i), truth=p["truth"], sampling_weight=p["sampling_weight"],
                              penalty_weight=p["penalty_weight"], truncation_strategy=p["truncation_strategy"],
                              fixed_right_cutoffs=p["fixed_right_cutoffs"]))
        random.seed(case)
        np.random.seed(case)
        fh = ref.FeatureHandler({"stride": 1, "window_step_ms": 10, "features": feats})
        batches = [fh.get_data("training", B, Tc, strategy, policy) for _ in range(2)]
        return batches, (random.random(), float(np.random.random()))


def main():
    from oracle.ref_data_shim import load_reference_data_module
    ref = load_reference_data_module()
    out = {"benchmark_store": [digest(a) for a in reference_benchmark_store(ref)], "fuzz": []}
    for case in range(FUZZ_CASES):
        batches, tail = reference_fuzz_case(ref, case)
        out["fuzz"].append({"batches": [[digest(a) for a in b] for b in batches], "tail": list(tail)})
    with open(FIXTURE, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
