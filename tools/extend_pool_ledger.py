#!/usr/bin/env python3
"""Static vector-instruction ledger of the pooled closest-hit pass (k_extend_pool: flat_prims_pool, csrc/jp_device.h; DESIGN.md section 5, "Pooled closest
hits") next to the loop it replaces (k_extend<2, FeatFlat>: flat_prims), from a `make -C jet-pbrt_amd/csrc asm` build, multiplied out with the per-wave
counts of tools/extend_pool_stats.py.  CPU only:
    python tools/extend_pool_ledger.py [jet-pbrt_amd/csrc/jp_kernels.s [jet-pbrt_amd/csrc/resource_usage.txt]]
Per kernel the blocks of the pass are put into classes by what they hold:
  box sweep      four leaves (24 v_sub_f32 from scalar plane operands)
  header         loads records and divides: in flat_prims the part of a trip every candidate pays (record, oa, two dot products, the division, the interval
                 compares); in the pooled pass the same for a dense round's 64 pairs, with the pair's decode and the owner's ray in front of it
  inside         the inside test (cross products, dot products, sign compares), by shape: runs when a lane of the wave passed the interval test
  list           the pooled pass's trip: ballot rank, ring address, the 16-bit store, the mask's next bit
  atomic         the 64-bit LDS minimum
  other          exec-mask bookkeeping, loop control, the pass's prologue and write-back
and the estimate is   today: trips x (header + hot share x inside[triangle]);   pooled: trips x list + rounds x (header + inside[triangle] + atomic) + 20,
for camera waves and bounce waves, weighted by their share of the frame's passes."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from shadow_pair_ledger import counts, read_kernels, resources

WANT = ("k_extend_pool", "k_extend<2, FeatFlat>")
# per-wave counts (tools/extend_pool_stats.py, profiles/extend_pool_stats.txt): share of the frame's passes (1 of 3.455 closest-hit rays a sample is a camera ray), trips, share of
# the trips with a lane past the interval test, dense rounds
WAVES = (("camera", 0.29, 6.05, 0.93, 3.46), ("bounce", 0.71, 10.2, 0.85, 3.9))


def classify(b):
    valu, _, lds, div = counts(b)
    has = lambda p: any(i.startswith(p) for i in b)
    if sum(1 for i in b if i.startswith("v_sub_f32")) == 24 and not lds:
        return "box sweep"
    if has("ds_write_b16"):
        return "list"
    if div and has("ds_read_b128"):
        return "header"
    if has("ds_min_u64") or has("ds_min_rtn_u64"):
        return "atomic"
    if valu >= 40 and not div:
        return "inside"
    return "other"


def main():
    asm = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "jet-pbrt_amd", "csrc", "jp_kernels.s")
    usage = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(asm), "resource_usage.txt")
    kernels = read_kernels(asm)
    res = resources(usage)
    names = subprocess.run(["c++filt"], input="\n".join(kernels), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    est = {}
    for mangled, name in zip(kernels, names):
        name = name.split("(")[0].replace("void ", "").replace("jp::Feat<false, true, true>", "FeatFlat").replace(" >", ">")
        if name not in WANT:
            continue
        r = res.get(mangled, {})
        print("%s: %s VGPRs, %s waves per SIMD, %s bytes of scratch per lane" % (name, r.get("vgpr", "?"), r.get("waves", "?"), r.get("scratch", "?")))
        by = {}
        for label, _, b in kernels[mangled]:
            c = classify(b)
            valu, salu, lds, div = counts(b)
            by.setdefault(c, []).append((label, valu, salu, lds, div))
            if c != "other":
                print("  %-10s %-10s %3d VALU %3d SALU %2d LDS %d division(s)" % (c, label, valu, salu, lds, div))
        other = sum(v for _, v, _, _, _ in by.get("other", []))
        print("  %-10s %d blocks, %d VALU in all (exec-mask bookkeeping, loop control, prologue, write-back, the counter's reduction)" % ("other", len(by.get("other", [])), other))
        # the triangle's inside test is the shorter of the two shapes'; the pooled kernel holds a second copy of the round for the last, partial one, and k_extend<2, FeatFlat> a
        # second loop for the 64-bit masks (the longer header): the Cornell box runs the shorter of each
        header = min(v for _, v, _, _, _ in by["header"]); inside = min(v for _, v, _, _, _ in by["inside"])
        if name == "k_extend_pool":
            lst = by["list"][0][1] + 4; atomic = by["atomic"][0][1]                         # + 4: the mask's next bit (two), the ballot's compare and the store's own compare
            est[name] = {}
            for w, _, trips, _, rounds in WAVES:
                est[name][w] = trips * lst + rounds * (header + inside + atomic) + 20
                print("  per %s pass: %.1f trips x %d (list) + %.1f rounds x (%d header + %d inside + %d atomic) + about 20 (prologue, write-back) = %.0f vector instructions"
                      % (w, trips, lst, rounds, header, inside, atomic, est[name][w]))
            print("  LDS per workgroup behind the primitive table: 4 waves x 2816 bytes (rays 2048, slots 512, ring 256) = 11264; with 2560 bytes of records 13824 a workgroup,"
                  " eight workgroups a CU: 110592 of 163840 bytes")
        else:
            est[name] = {}
            for w, _, trips, hot, _ in WAVES:
                est[name][w] = trips * (header + hot * inside)
                print("  per %s pass: %.1f trips x (%d header + %.2f x %d inside) = %.0f vector instructions" % (w, trips, header, hot, inside, est[name][w]))
        print()
    if len(est) == 2:
        mix = 0.0
        for w, share, _, _, _ in WAVES:
            a, b = est["k_extend<2, FeatFlat>"][w], est["k_extend_pool"][w]
            mix += share * (b - a)
            print("primitive phase per 64-ray %s pass: today %.0f, pooled %.0f: %+.0f vector instructions" % (w, a, b, b - a))
        print("the frame's mix (%s): %+.0f vector instructions a pass, %.1f %% of the 1,106 a pass of k_extend<2, FeatFlat> runs"
              % (", ".join("%.2f %s" % (share, w) for w, share, _, _, _ in WAVES), mix, 100.0 * mix / 1106.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
