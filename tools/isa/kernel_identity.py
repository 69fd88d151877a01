"""Device-code identity listing of a built libmww_hip.so: is the device code of two builds the same, kernel by kernel?

For every gfx950 code object in the library one line per kernel: demangled name, sha256 of its disassembly (addresses, symbol
offsets and comments stripped), .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size from the
code-object metadata.  With --against OTHER the other library is listed the same way and compared: a code object that holds
the same kernels with the same lines in both (a unit the change did not touch) gets one line, the sha256 over its kernel lines
(not over the file: a code object carries a __hip_cuid_<hash> symbol derived from its unit's path); every other kernel is
compared by its own line, and the verdict is printed last.

One difference is normalised away: the literal of the s_getpc_b64 / s_add_u32 / s_addc_u32 idiom, the pc-relative distance
from a kernel to a data symbol of its code object, which changes when kernels move between code objects.  The listing says
per kernel how many were masked.  The s_nop padding behind a kernel's last instruction (alignment of what follows it in the code
object) is not part of the hash either.  Host-side only: it inspects files and runs nothing on a GPU.

usage: python tools/isa/kernel_identity.py LIB [--against OTHER] [--arch gfx950]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, arch, tmp):
    """extracts the device code objects of `lib` for `arch` into tmp; returns their paths in library order"""
    link = os.path.join(tmp, "lib.so")
    os.symlink(os.path.abspath(lib), link)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", link, cwd=tmp)
    objs = [f for f in os.listdir(tmp) if f.startswith("lib.so.") and f.endswith(arch)]
    return [os.path.join(tmp, f) for f in sorted(objs, key=lambda f: int(re.match(r"lib\.so\.(\d+)", f).group(1)))]


def kernel_meta(obj):
    """kernel symbol -> (vgpr, sgpr, lds, scratch) from the AMDGPU metadata note"""
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", obj)
    meta = {}
    for chunk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, chunk).group(1))
        sym = re.search(r"\.symbol:\s+'?([^'\s]+?)\.kd'?\s", chunk).group(1)
        meta[sym] = (g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"))
    return meta


def kernel_hashes(obj, names):
    """kernel symbol -> (sha256 of the normalised disassembly, number of masked pc-relative literals)"""
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj)
    out, cur, since_getpc = {}, None, 99
    for ln in dis.split("\n"):
        m = re.match(r"(?:[0-9a-f]+ )?<(\S+)>:$", ln)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                out[cur] = [[], 0]
            since_getpc = 99
            continue
        if cur is None or not ln.strip():
            continue
        ins = re.sub(r"<[^>]*>", "", ln.split("//")[0]).split()
        if not ins or ins[0] == "...":   # (zero fill behind the code object's last kernel)
            continue
        since_getpc += 1
        if ins[0] == "s_getpc_b64":
            since_getpc = 0
        elif since_getpc <= 4 and ins[0] in ("s_add_u32", "s_addc_u32") and re.fullmatch(r"(0x[0-9a-f]+|-?\d+)", ins[-1]):
            ins[-1] = "PCREL"
            out[cur][1] += 1
        out[cur][0].append(" ".join(ins))
    res = {}
    for k, (body, n) in out.items():
        while body and body[-1].split()[0] in ("s_nop", "s_code_end"):   # padding behind the kernel's last instruction
            body.pop()
        res[k] = (hashlib.sha256("\n".join(body).encode()).hexdigest(), n)
    return res


def listing(lib, arch):
    """[(object sha256, {demangled kernel name: line})] in library order"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in code_objects(lib, arch, tmp):
            with open(obj, "rb") as fh:
                osha = hashlib.sha256(fh.read()).hexdigest()
            meta = kernel_meta(obj)
            hashes = kernel_hashes(obj, set(meta))
            syms = sorted(meta)
            dem = run("c++filt", *syms).split("\n") if syms else []
            lines = {}
            for s, d in zip(syms, dem):
                sha, masked = hashes[s]
                lines[d] = "%s sha256=%s vgpr=%d sgpr=%d lds=%d scratch=%d pcrel_masked=%d" % ((d.replace("mww::", ""), sha) + meta[s] + (masked,))
            res.append((osha, lines))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib")
    ap.add_argument("--against", help="the library to compare with (e.g. the parent commit's build)")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    mine = listing(args.lib, args.arch)
    if not args.against:
        for osha, lines in mine:
            print("# code object sha256=%s kernels=%d" % (osha, len(lines)))
            for d in sorted(lines):
                print(lines[d])
        return 0
    other = listing(args.against, args.arch)
    # a code object that holds the same kernels, line for line, in both libraries (a unit the change did not touch) gets one line
    digest = lambda lines: hashlib.sha256("\n".join(lines[d] for d in sorted(lines)).encode()).hexdigest()
    other_objs = {digest(lines) for _, lines in other}
    same_objs = [lines for _, lines in mine if digest(lines) in other_objs]
    for lines in same_objs:
        print("code object of %d kernels (%s ...): sha256 over its kernel lines %s, equal in both libraries" % (len(lines), sorted(lines)[0].replace("mww::", "")[:50], digest(lines)))
    mine_objs = {digest(lines) for _, lines in mine}
    a, b = {}, {}
    for _, lines in mine:
        if digest(lines) not in other_objs:
            a.update(lines)
    for _, lines in other:
        if digest(lines) not in mine_objs:
            b.update(lines)
    bad = 0
    for d in sorted(set(a) | set(b)):
        if d not in a or d not in b:
            print("ONLY IN %s: %s" % ("THIS" if d in a else "OTHER", d))
            bad += 1
        elif a[d] != b[d]:
            print("DIFFERENT: %s\n   this:  %s\n   other: %s" % (d, a[d], b[d]))
            bad += 1
        else:
            print(a[d])
    print("# %d code objects with equal kernel lines; %d kernels in the other code objects compared line by line, %d pc-relative literals masked; %d differ or are missing"
          % (len(same_objs), len(set(a) | set(b)), sum(int(l.rsplit("=", 1)[1]) for l in a.values()), bad))
    print("# verdict: %s" % ("IDENTICAL device code" if bad == 0 else "DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
