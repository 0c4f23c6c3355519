#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two `make -C jet-pbrt_amd/csrc asm` builds have in common, modulo label and function
numbering (labels, comments and directives dropped).  CPU only:
    python tools/asm_kernel_diff.py OLD/jp_kernels.s NEW/jp_kernels.s
Prints one line per kernel of OLD that differs or is missing in NEW, then a summary; exit status 1 if any does."""
import re
import sys


def kernels(path):
    out, cur, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        s = re.sub(r"\.L\w+", ".L", s)                    # block labels and constants pools: numbering only
        body.append(s)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(a):
        if name not in b:
            print("missing  %s" % name); bad += 1
        elif a[name] != b[name]:
            print("differs  %s (%d vs %d instructions)" % (name, len(a[name]), len(b[name]))); bad += 1
    print("%d kernels of the old build, %d identical, %d differ or are missing; %d kernels only in the new build"
          % (len(a), len(a) - bad, bad, len(set(b) - set(a))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
