"""Which block-kernel instantiations did the GPU sweep actually launch?  The form rules of tests/block_table_sweep.py restate the
C++ dispatch, and a launcher that finds no instantiation of a form falls back without a word (wide -> narrow, x6 -> exact), so
the plan's claim is checked against a kernel trace of the sweep:

    rocprofv3 --kernel-trace --stats -d <dir> -- python -m pytest tests/test_block_table_sweep_gpu.py -q -m gpu
    python tools/table_sweep_kernels.py <dir, kernel_stats.csv or rocpd .db ...> [--out profiles/block_table_sweep_kernels.txt]

Reads every *kernel_stats.csv and rocpd database (*.db) under the arguments, maps the demangled template names (``void mww::bwd_blockw_kernel<48, 48, 21,
true, 512, false, false>(mww::BwdBlockArgs)``) onto the inventory of the built library and prints the instantiations that never
ran (and any launched block kernel outside the inventory).  Exit status 1 when one is missing."""
import argparse
import csv
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import block_table_sweep as bts   # noqa: E402
from microwakeword_amd import native   # noqa: E402

_NAME = re.compile(r"mww::((?:fwd|bwd)_(?:first|block)w?_kernel<[^>]*>)")


def launched(paths):
    """{instantiation: calls} of the block kernels in the traces under `paths`: rocprofv3's *kernel_stats.csv (--stats with
    -f csv) or its rocpd database (*.db, the default output format)."""
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += sorted(glob.glob(os.path.join(p, "**", "*kernel_stats.csv"), recursive=True))
            files += sorted(glob.glob(os.path.join(p, "**", "*.db"), recursive=True))
        else:
            files.append(p)
    if not files:
        raise SystemExit("no kernel_stats.csv or rocpd .db under %s" % paths)
    rows = []
    for f in files:
        if f.endswith(".db"):
            with sqlite3.connect(f) as db:
                rows += db.execute("SELECT name, COUNT(*) FROM kernels GROUP BY name").fetchall()
        else:
            with open(f, newline="") as fh:
                rows += [(r["Name"], int(r["Calls"])) for r in csv.DictReader(fh)]
    out = {}
    for name, calls in rows:
        m = _NAME.search(name)
        if m:
            out[m.group(1)] = out.get(m.group(1), 0) + int(calls)
    return out, files


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = native.NativeLib.get()
    inv = bts.inventory(lib)
    ran, files = launched(args.paths)
    missing = sorted(inv - set(ran))
    extra = sorted(set(ran) - inv)
    lines = ["block-kernel instantiations launched by tests/test_block_table_sweep_gpu.py (%d cases), from a rocprofv3 --kernel-trace --stats run on an MI355X"
             % len(bts.plan(lib)),
             "library %s" % lib.version(),
             "inventory (tests/block_table_sweep.py): %d instantiations; launched: %d of them; missing: %d; outside the inventory: %d"
             % (len(inv), len(inv & set(ran)), len(missing), len(extra)), ""]
    lines.append("per launcher (inventory / launched):")
    for name in sorted({bts.launcher_of(i) for i in inv}):
        n_inv = sum(1 for i in inv if bts.launcher_of(i) == name)
        n_ran = sum(1 for i in inv if bts.launcher_of(i) == name and i in ran)
        lines.append("  %-20s %4d / %4d" % (name, n_inv, n_ran))
    lines.append("")
    lines += ["MISSING " + i for i in missing] + ["OUTSIDE " + i for i in extra]
    lines.append("")
    lines.append("launched instantiations (calls):")
    lines += ["  %s %d" % (i, ran[i]) for i in sorted(ran)]
    text = "\n".join(lines) + "\n"
    print(text if len(text) < 4000 else "\n".join(lines[:12 + len(missing) + len(extra)]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
