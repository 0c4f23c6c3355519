#!/usr/bin/env python3
"""Static ledger of the k_shade<true, true, true, *> instances (lean and generic) and k_shade_lean_one from a `make -C jet-pbrt_amd/csrc asm` build:
vector instructions, expanded IEEE divisions (one v_div_fixup_f32 each), v_sqrt_f32, v_rcp_f32, and the resource-usage remarks.  CPU only:
    python tools/shade_cuts_ledger.py [DIR with jp_kernels.s and resource_usage.txt]   (default: jet-pbrt_amd/csrc)"""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import asm_kernel_diff as A
import resource_table as R


def main():
    d = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "jet-pbrt_amd", "csrc")
    ks = A.kernels(os.path.join(d, "jp_kernels.s"))
    if not ks:
        sys.exit("no kernels in %s" % os.path.join(d, "jp_kernels.s"))
    names = dict(zip(ks, [R.short(n) for n in R.demangle(list(ks))]))
    res = {}
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "resource_table.py"), os.path.join(d, "resource_usage.txt")], stdout=subprocess.PIPE, text=True, check=True).stdout
    for line in out.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            res[m.group(1).strip()] = [int(x) for x in m.groups()[1:]]
    print("%-40s %6s %5s %6s %5s | %5s %8s %10s %7s" % ("kernel", "VALU", "div", "v_sqrt", "v_rcp", "VGPR", "scratch", "waves/SIMD", "LDS(B)"))
    for mangled in sorted(ks, key=lambda k: names[k]):
        n = names[mangled]
        if not (n.startswith("k_shade<true, true, true, ") or n == "k_shade_lean_one"):
            continue
        body = ks[mangled]
        op = [s.split()[0] for s in body]
        r = res.get(n, [-1] * 6)
        print("%-40s %6d %5d %6d %5d | %5d %8d %10d %7d" % (n, sum(o.startswith("v_") for o in op), op.count("v_div_fixup_f32"), sum(o.startswith("v_sqrt_f32") for o in op),
                                                          sum(o.startswith("v_rcp_f32") for o in op), r[0], r[3], r[4], r[5]))


if __name__ == "__main__":
    main()
