#!/usr/bin/env python3
"""Compare two tools/dump_isa.py dumps kernel by kernel (no GPU needed).

  python tools/dump_isa.py OLD . (with ISA_OBJDIR at the other build's objects)    python tools/dump_isa.py NEW .
  python tools/compare_isa.py OLD NEW

For every kernel of OLD: the row of resources.tsv (VGPRs, AGPRs, SGPRs, LDS, scratch) and the instruction stream (<kernel>.s;
dump_isa.py already strips addresses and encodings, branches are relative) must be the same in NEW.  One thing is normalised and
nothing else: the literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 is the distance to another symbol of the code
object and moves when the object's layout does.  Kernels that exist only in NEW are listed, not compared.  Exit status 1 when a kernel
of OLD differs or is missing."""
import os
import re
import sys


def resources(d):
    rows = {}
    with open(os.path.join(d, "resources.tsv")) as f:
        next(f)
        for line in f:
            c = line.rstrip("\n").split("\t")
            rows[(c[0], c[1])] = tuple(c[2:])
    return rows


def stream(path):
    out, pc = [], 0
    with open(path) as f:
        for line in f:
            if line.startswith(";"):
                continue                                    # dump_isa.py's header: name, resources, instruction histogram
            s = line.strip()
            if not s:
                continue
            op = s.split()[0]
            if op == "s_getpc_b64":
                pc = 2
            elif pc and op in ("s_add_u32", "s_addc_u32"):
                s = re.sub(r",\s*(0x[0-9a-fA-F]+|-?\d+)\s*$", ", <pcrel>", s)
                pc -= 1
            out.append(s)
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    ro, rn = resources(old), resources(new)
    so = {f for f in os.listdir(old) if f.endswith(".s")}
    sn = {f for f in os.listdir(new) if f.endswith(".s")}
    bad = []
    for k in sorted(ro):
        if k not in rn:
            bad.append(f"missing in NEW: {k[0]} {k[1]}")
        elif ro[k] != rn[k]:
            bad.append(f"resources differ: {k[0]} {k[1]}: {ro[k]} -> {rn[k]}")
    pcrel = 0
    for f in sorted(so):
        if f not in sn:
            bad.append(f"no instruction stream in NEW: {f}")
            continue
        a, b = stream(os.path.join(old, f)), stream(os.path.join(new, f))
        pcrel += any("<pcrel>" in s for s in a)
        if a != b:
            bad.append(f"instruction stream differs: {f}")
    print(f"kernels compared: {len(ro)} resource rows, {len(so)} instruction streams ({pcrel} with a normalised pc-relative literal)")
    print(f"kernels only in NEW: {len(set(rn) - set(ro))} resource rows, {len(sn - so)} instruction streams")
    print(f"kernels differing: {len(bad)}")
    for b in bad:
        print("  " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
