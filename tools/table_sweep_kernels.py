"""Which block-kernel instantiations did the GPU sweep actually launch?  The form rules of tests/block_table_sweep.py restate the
C++ dispatch, and a launcher that finds no instantiation of a form falls back without a word (wide -> narrow, x6 -> exact), so
the plan's claim is checked against a kernel trace of the sweep:

    rocprofv3 --kernel-trace --stats -d <dir> -- python -m pytest tests/test_block_table_sweep_gpu.py -q -m gpu
    python tools/table_sweep_kernels.py <dir, kernel_stats.csv or rocpd .db ...> [--out profiles/block_table_sweep_kernels.txt]

Reads every *kernel_stats.csv and rocpd database (*.db) under the arguments, maps the demangled template names (``void mww::bwd_blockw_kernel<48, 48, 21,
true, 512, false, false>(mww::BwdBlockArgs)``) onto the inventory of the built library and prints the instantiations that never
ran (and any launched block kernel outside the inventory).  Exit status 1 when one is missing.

``--graph``: the same for the conv/BN graph kernels - a trace of tests/test_graph_table_sweep_gpu.py against the inventory of
tests/graph_table_sweep.py (read from csrc/graph_launch.hip.h); the instantiations no flag set reaches (UNREACHABLE) are listed
apart with their reasons.  The kernel trace runs on its own, not combined with counters:

    rocprofv3 --kernel-trace --stats -d <dir> -- python -m pytest tests/test_graph_table_sweep_gpu.py -q -m gpu
    python tools/table_sweep_kernels.py --graph <dir> [--out profiles/graph_table_sweep_kernels.txt]"""
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
_GRAPH_NAME = re.compile(r"(?:mww::)?\b(g(?:conv|dw|res|head|bn)\w*_kernel)\b")
_GSHAPE = re.compile(r",?\s*(?:mww::)?GShape<([^<>]*)>\s*")


def graph_instantiation(name, shapes):
    """A demangled graph-kernel name of a trace (``void mww::gconv_kernel<24, 0, mww::GShape<5, 1, 40, 40, 0, 0, 0, 0> >(mww::GConvArgs)``)
    as graph_table_sweep names it (``gconv_kernel<24, 0, GSh1>``; the run-time shape GShape<0, ...> is the default argument and
    dropped), or None for another kernel."""
    m = _GRAPH_NAME.search(name)
    if not m:
        return None
    rest = name[m.end():]
    if not rest.startswith("<"):
        return m.group(1)
    depth = 0
    for i, ch in enumerate(rest):
        depth += (ch == "<") - (ch == ">")
        if depth == 0:
            break
    args = rest[1:i]

    def shape(mm):
        row = tuple(int(v) for v in mm.group(1).split(","))
        row += (0,) * (8 - len(row))
        if not any(row):
            return ""
        ids = [sid for sid, r in shapes.items() if tuple(r) == row]
        return ", GSh%d" % ids[0] if ids else ", GShape<%s>" % ", ".join(map(str, row))
    args = _GSHAPE.sub(shape, args)
    return "%s<%s>" % (m.group(1), ", ".join(a.strip() for a in args.split(",")))


def launched(paths, name_of=None):
    """{instantiation: calls} of the block kernels (name_of: of the kernels it names) in the traces under `paths`: rocprofv3's
    *kernel_stats.csv (--stats with -f csv) or its rocpd database (*.db, the default output format)."""
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
        if name_of is not None:
            inst = name_of(name)
        else:
            m = _NAME.search(name)
            inst = m.group(1) if m else None
        if inst:
            out[inst] = out.get(inst, 0) + int(calls)
    return out, files


def graph_main(args):
    import graph_table_sweep as gts
    tabs = gts.tables()
    inv = gts.inventory()
    unreachable = {k: why for k, why in gts.UNREACHABLE.items() if isinstance(k, str)}
    ran, files = launched(args.paths, lambda n: graph_instantiation(n, tabs["shapes"]))
    reach = inv - set(unreachable)
    missing = sorted(reach - set(ran))
    extra = sorted(set(ran) - reach)
    lines = ["conv/BN graph kernel instantiations launched by tests/test_graph_table_sweep_gpu.py (%d cases), from a rocprofv3 --kernel-trace --stats run on an MI355X"
             % len(gts.plan()),
             "inventory (tests/graph_table_sweep.py, from csrc/graph_launch.hip.h): %d instantiations, %d of them out of reach of any flag set; "
             "launched: %d of the other %d; missing: %d; outside the inventory: %d"
             % (len(inv), len(unreachable), len(reach & set(ran)), len(reach), len(missing), len(extra)), ""]
    lines.append("per launcher (reachable inventory / launched):")
    for name in sorted({gts.launcher_of(i) for i in inv}):
        mine = [i for i in reach if gts.launcher_of(i) == name]
        lines.append("  %-28s %4d / %4d" % (name, len(mine), sum(1 for i in mine if i in ran)))
    lines.append("")
    lines += ["MISSING " + i for i in missing] + ["OUTSIDE " + i for i in extra]
    lines.append("")
    lines.append("UNREACHABLE (graph_table_sweep.UNREACHABLE: in the tables, launched by no Inception or MixedNet flag set):")
    lines += ["  %s: %s" % (k, unreachable[k]) for k in sorted(unreachable)]
    lines.append("")
    lines.append("launched instantiations (calls):")
    lines += ["  %s %d" % (i, ran[i]) for i in sorted(ran)]
    text = "\n".join(lines) + "\n"
    print(text if len(text) < 4000 else "\n".join(lines[:22 + len(missing) + len(extra)]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if missing or extra else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--out")
    ap.add_argument("--graph", action="store_true", help="the conv/BN graph kernels (tests/graph_table_sweep.py)")
    args = ap.parse_args()
    if args.graph:
        return graph_main(args)
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
