#!/usr/bin/env python3
"""Compare two device-only assembly listings (hipcc --cuda-device-only -S) kernel by kernel.

    compare_listings.py A.s B.s [--match k_fiber_pair]

For every kernel whose symbol contains the --match string, the instruction lines and labels of its body and the lines of
its .amdhsa_kernel descriptor are compared with comments (everything from ';'), blank lines and the per-translation-unit
__hip_cuid_* symbol left out.  Block labels carry the number of the function in its translation unit (.LBB52_5); it is left out
too, so that a kernel added to the file does not make every kernel behind it differ.  Prints one line per kernel that differs and a total; the exit status is 0 when every
kernel is identical and both listings hold the same kernels.
"""
import argparse
import re
import sys


def kernels(path, match):
    """symbol -> list of the significant lines of its body and its kernel descriptor"""
    out, cur, names = {}, None, set()
    with open(path) as f:
        lines = f.read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    for ln in lines:
        code = ln.split(";", 1)[0].rstrip()
        if not code.strip() or "__hip_cuid_" in code:
            continue
        m = re.match(r"(\S+):$", code)
        if m and m.group(1) in names:  # the body starts at the kernel's own label ...
            cur = m.group(1) if match in m.group(1) else None
            if cur:
                out[cur] = []
            continue
        if cur and re.match(r"\s*\.(Lfunc_end\d+:|size\s|section\s|text$)", code):  # ... and ends with the function
            cur = None
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", code)
        if m:
            cur = m.group(1) if match in m.group(1) else None
        if cur:
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", code.strip()))
        if re.match(r"\s*\.end_amdhsa_kernel", code):
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--match", default="k_fiber_pair")
    args = ap.parse_args()
    ka, kb = kernels(args.a, args.match), kernels(args.b, args.match)
    bad = 0
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"only in {'A' if name in ka else 'B'}: {name}")
            bad += 1
        elif ka[name] != kb[name]:
            la, lb = ka[name], kb[name]
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"differs: {name} ({len(la)} / {len(lb)} lines, first at {first}: "
                  f"{la[first] if first < len(la) else '<end>'!r} / {lb[first] if first < len(lb) else '<end>'!r})")
            bad += 1
    n = len(set(ka) | set(kb))
    print(f"{n} kernels compared, {n - bad} identical, {sum(len(v) for v in ka.values())} lines")
    return 1 if bad or not n else 0


if __name__ == "__main__":
    sys.exit(main())
