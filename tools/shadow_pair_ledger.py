#!/usr/bin/env python3
"""Static vector-instruction ledger of the two-rays-in-one-pass shadow walk (k_shadow_pair: flat_boxes_lean_pair / flat_prims_pair, csrc/jp_device.h) next
to the walk it replaces (k_shadow<2, FeatFlat>), from a `make -C jet-pbrt_amd/csrc asm` build.  CPU only:
    python tools/shadow_pair_ledger.py [jet-pbrt_amd/csrc/jp_kernels.s [jet-pbrt_amd/csrc/resource_usage.txt]]
Per kernel it prints
  * the box sweeps: every basic block that tests four leaves (24 v_sub_f32 from scalar plane operands) with its VALU count per leaf -- in k_shadow_pair the
    sweep that serves two rays, and the single-ray sweeps behind the odd last ray (the 32-bit lean one and the 64-bit copy for > 32 primitives);
  * the primitive loops: the header block of every any-hit loop (it loads the record and divides) and the blocks of that loop in text order, each with
    its VALU / SALU / LDS counts and divisions.  The header is what every candidate pays (the reject path: record address, record, oa, dot(n, oa), one
    dot(n, d) + division + interval compares per ray); the blocks behind it run only when the interval test passes (ob, oc, the cross products, the dot
    products and sign compares, split by shape); the short blocks are the exec-mask bookkeeping of the loop;
  * VGPRs, waves per SIMD and scratch from the resource-usage remarks."""
import collections
import os
import re
import subprocess
import sys

WANT = ("k_shadow_pair", "k_shadow<2, FeatFlat>")
HERE = os.path.dirname(os.path.abspath(__file__))


def read_kernels(path):
    """mangled name -> list of blocks (label, loop header label or None, [mnemonic ...]); a block ends at a label, a `; %bb.N:` mark or a branch"""
    cur, out = None, collections.OrderedDict()
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1); out[cur] = [["entry", None, []]]
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(?:(\.LBB\w+):|; %(bb\.\d+):)(.*)$", line)
        if m:
            h = re.search(r"Header=(BB\w+)", m.group(3))
            own = re.search(r"Loop Header", m.group(3))
            label = m.group(1) or m.group(2)
            out[cur].append([label, (".L" + h.group(1)) if h else (label if own else None), []])
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith("."):
            out[cur][-1][2].append(s.split()[0])
    return out


def counts(b):
    valu = sum(1 for i in b if i.startswith("v_"))
    salu = sum(1 for i in b if i.startswith("s_") and not i.startswith(("s_load", "s_waitcnt", "s_nop", "s_cbranch", "s_branch")))
    lds = sum(1 for i in b if i.startswith("ds_"))
    div = sum(1 for i in b if i.startswith("v_div_fixup"))
    return valu, salu, lds, div


def resources(path):
    """kernel name -> (VGPRs, scratch bytes, waves per SIMD) from hipcc's -Rpass-analysis=kernel-resource-usage remarks"""
    res, name = {}, None
    if not os.path.exists(path):
        return res
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); res[name] = {}
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


def main():
    asm = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "jet-pbrt_amd", "csrc", "jp_kernels.s")
    usage = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(asm), "resource_usage.txt")
    kernels = read_kernels(asm)
    res = resources(usage)
    names = subprocess.run(["c++filt"], input="\n".join(kernels), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for mangled, name in zip(kernels, names):
        name = name.split("(")[0].replace("void ", "").replace("jp::Feat<false, true, true>", "FeatFlat").replace(" >", ">")
        if name not in WANT:
            continue
        r = res.get(mangled, {})
        print("%s: %s VGPRs, %s waves per SIMD, %s bytes of scratch per lane" % (name, r.get("vgpr", "?"), r.get("waves", "?"), r.get("scratch", "?")))
        blocks = kernels[mangled]
        for label, _, b in blocks:
            if sum(1 for i in b if i.startswith("v_sub_f32")) == 24 and not any(i.startswith("ds_") for i in b):
                valu, salu, _, _ = counts(b)
                rays = sum(1 for i in b if i.startswith("v_cmp_le_f32")) // 4                # one slack compare per leaf and ray
                print("  box sweep %-10s four leaves, %d ray(s): %3d VALU = %5.2f per leaf (%5.2f per leaf and ray), %2d SALU, %d SMEM"
                      % (label, rays, valu, valu / 4.0, valu / 4.0 / max(rays, 1), salu, sum(1 for i in b if i.startswith("s_load"))))
        for label, _, b in blocks:
            if not (any(i.startswith("ds_read_b128") for i in b) and any(i.startswith("v_div_fixup") for i in b)):
                continue
            body = [(l, bb) for l, h, bb in blocks if h == label or l == label]
            print("  primitive loop %s" % label)
            tv = ts = 0
            for l, bb in body:
                valu, salu, lds, div = counts(bb)
                tv += valu; ts += salu
                role = "header: every candidate" if l == label else ("bookkeeping" if valu < 10 else "interval passed")
                print("    %-10s %3d VALU %3d SALU %2d LDS %d division(s)   %s" % (l, valu, salu, lds, div, role))
            print("    %-10s %3d VALU %3d SALU over the whole loop body" % ("sum", tv, ts))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
