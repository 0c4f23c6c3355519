#!/usr/bin/env python3
"""Per-leaf vector-instruction ledger of the tiny-scene box phase (flat_boxes / flat_boxes_lean, csrc/jp_device.h), from a
`make -C jet-pbrt_amd/csrc asm` listing.  CPU only:
    python tools/flat_boxes_ledger.py [jet-pbrt_amd/csrc/jp_kernels.s]
In every k_extend<2..>, k_shadow<2..> and k_trace instance of the tiny-scene walk it finds the basic blocks that test four leaves (24 v_sub_f32
from scalar plane operands) and prints their VALU count per leaf with the instruction mix (two-operand v_min / v_max: 6 per leaf for the
slabs, + 1 against tmin, + 1 against tmax where it is clamped).  A block with 2 scalar loads is the 64-bit-mask copy for > 32 primitives."""
import collections
import os
import re
import subprocess
import sys

WANT = re.compile(r"k_(extend|shadow)<2|k_trace(<2>|_flat)")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "jet-pbrt_amd", "csrc", "jp_kernels.s")
    cur, blocks = None, collections.OrderedDict()
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1); blocks[cur] = [[]]
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if re.match(r"^\.LBB\w+:", s):
            blocks[cur].append([])
        elif s and not s.startswith("."):
            blocks[cur][-1].append(s.split()[0])
            if s.startswith(("s_cbranch", "s_branch")):
                blocks[cur].append([])
    names = subprocess.run(["c++filt"], input="\n".join(blocks), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for mangled, name in zip(blocks, names):
        name = name.split("(")[0].replace("void ", "").replace("jp::Feat<false, true, true>", "FeatFlat")
        if not WANT.search(name):
            continue
        for b in blocks[mangled]:
            if sum(1 for i in b if i.startswith("v_sub_f32")) != 24:
                continue
            valu = [i for i in b if i.startswith("v_")]
            mix = collections.Counter(re.sub(r"_e(32|64)$", "", i) for i in valu)
            two = mix["v_min_f32"] + mix["v_max_f32"]
            print("%-24s four-leaf block: %3d VALU = %5.2f per leaf, %2d SALU, %2d SMEM | two-operand min/max per leaf %.2f | %s"
                  % (name, len(valu), len(valu) / 4.0, sum(1 for i in b if i.startswith("s_") and not i.startswith(("s_load", "s_waitcnt", "s_nop"))),
                     sum(1 for i in b if i.startswith("s_load")), two / 4.0, " ".join("%s:%d" % kv for kv in sorted(mix.items()))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
