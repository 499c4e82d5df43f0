#!/usr/bin/env python3
"""Do two builds hold the same gfx950 kernels?  For a change of host code only: the device code must come out the same.

    python tools/kernel_diff.py <build_a> <build_b>      (directories of *.hip.o, or two single objects / libraries)

Prints, and exits non-zero on, any of: a kernel symbol in one build only; a metadata field (registers, LDS, scratch, spills) that
differs; a kernel whose disassembly differs (llvm-objdump -d of the unbundled code objects, addresses and symbol order ignored).
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402


def objects(path):
    return sorted(glob.glob(os.path.join(path, "*.hip.o"))) if os.path.isdir(path) else [path]


def disassembly(paths):
    """(object, kernel symbol) -> instruction text (the `// address: encoding` comments and branch-target labels dropped)"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for p in paths:
            for co in kr.code_objects(p, tmp):
                txt = subprocess.run([kr._tool("llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
                name = None
                for line in txt.splitlines():
                    m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                    if m:
                        name = (os.path.basename(p), m.group(1))
                        out[name] = []
                    elif name and line.startswith("\t") and line.strip() != "...":   # ("...": zero padding up to the next symbol)
                        out[name].append(re.sub(r"\s*<\S+>$", "", line.split("//")[0]).strip())
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = objects(sys.argv[1]), objects(sys.argv[2])
    ka, kb = ({(k["file"], k["name"]): k for k in kr.collect(p)} for p in (a, b))   # (unnamed-namespace kernels: one per object)
    bad = 0
    for tag, only in (("only in A", sorted(set(ka) - set(kb))), ("only in B", sorted(set(kb) - set(ka)))):
        for n, d in zip(only, kr.demangle([n[1] for n in only])):
            print("%s: %s: %s" % (tag, n[0], d))
            bad += 1
    both = sorted(set(ka) & set(kb))
    for n in both:
        diff = ["%s %s -> %s" % (f, ka[n].get(f), kb[n].get(f)) for f in kr.FIELDS if ka[n].get(f) != kb[n].get(f)]
        if diff:
            print("metadata: %s: %s" % (ka[n]["demangled"], ", ".join(diff)))
            bad += 1
    da, db = disassembly(a), disassembly(b)
    for n in both:
        if n not in da or n not in db:
            print("no disassembly: %s" % ka[n]["demangled"])
            bad += 1
        elif da[n] != db[n]:
            first = next((i for i, (x, y) in enumerate(zip(da[n], db[n])) if x != y), min(len(da[n]), len(db[n])))
            print("code: %s: %d / %d instructions, first difference at %d" % (ka[n]["demangled"], len(da[n]), len(db[n]), first))
            bad += 1
    print("%d kernels in A, %d in B, %d in both, %d differences" % (len(ka), len(kb), len(both), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
