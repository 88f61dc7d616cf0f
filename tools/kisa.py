#!/usr/bin/env python3
"""usage: tools/kisa.py FILE.hip PARENT_TREE [THIS_TREE] -- compare the gfx950 code of one kernel file between two trees.

Compiles csrc/FILE.hip of both trees to assembly with the flags the Makefile uses for that file and prints, per kernel
instantiation: VGPRs, AGPRs, LDS bytes, scratch, occupancy and the instruction count of either tree, whether the
opcode histograms are equal, and whether the instruction streams are equal once comments, labels' numbers and symbol
names are stripped.  Compile only: no GPU.  (tools/kres.sh prints the resources of one tree.)"""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

RES = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"), ("occ", "Occupancy"))


def assembly(tree, name):
    csrc = os.path.join(tree, "magellanmapper_amd", "csrc")
    obj = "_obj/" + name.replace(".hip", ".o")
    cmds = subprocess.run(["make", "-C", csrc, "-n", "-B", obj], capture_output=True, text=True, check=True).stdout
    cmd = [l for l in cmds.splitlines() if " -c " in l and name in l][0].split()
    cmd = cmd[:cmd.index("-c")] + ["--cuda-device-only", "-S", name, "-o", "-"]
    return subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stdout


def kernels(asm):
    """demangled name -> (resources, opcode histogram, digest of the normalised stream)"""
    out, name, ops, norm = {}, None, None, None
    for line in asm.splitlines():
        m = re.match(r"(\w+):\s", line + " ")
        if m and ops is None and ("\t.type\t%s,@function" % m.group(1)) in asm:
            name, ops, norm, res = m.group(1), collections.Counter(), hashlib.sha1(), {}
            continue
        if ops is None:
            continue
        m = re.match(r"; (\w+): (\d+)", line)
        if m:
            res[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":         # the last figure of a function's summary
                short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
                short = re.sub(r"^void ", "", short.replace("(anonymous namespace)::", "")).split("(")[0]
                out[short] = ({k: res.get(v, 0) for k, v in RES}, ops, norm.hexdigest())
                ops = None
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        ops[code.split()[0]] += 1
        # (.LBB<function>_ and .Lpost_getpc<n> count through the file: they move with the order the kernels are emitted in)
        code = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\b_Z\w+", "SYM", code)))
        norm.update(code.encode() + b"\n")
    return out


def main():
    name, parent, this = sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(__file__), "..")
    a, b = kernels(assembly(parent, name)), kernels(assembly(this, name))
    print("# %s: parent -> this tree   (= : equal to the parent)" % name)
    print("# %-44s %9s %5s %7s %7s %4s %15s %6s %5s %6s" % ("kernel", "vgpr", "agpr", "lds", "scratch", "occ", "instructions", "delta", "hist", "stream"))
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("  %-44s only in %s" % (k[:44], "parent" if k in a else "this tree"))
            continue
        (ra, ha, da), (rb, hb, db) = a[k], b[k]
        na, nb = sum(ha.values()), sum(hb.values())
        cols = ["=" if ra[f] == rb[f] else "%d>%d" % (ra[f], rb[f]) for f, _ in RES]
        print("  %-44s %9s %5s %7s %7s %4s %15s %+5.1f%% %5s %6s" % (
            k[:44], "%s(%d)" % (cols[0], rb["vgpr"]), cols[1], cols[2], cols[3], "%s(%d)" % (cols[4], rb["occ"]),
            "%d>%d" % (na, nb), 100.0 * (nb - na) / na, "=" if ha == hb else "diff", "=" if da == db else "diff"))


if __name__ == "__main__":
    main()
