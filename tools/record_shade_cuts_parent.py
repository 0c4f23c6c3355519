#!/usr/bin/env python3
"""Record tests/golden/shade_cuts_parent.npz: the films and ray counts of the JP_LIGHTS_POWER_ONE and JP_ESTIMATOR_MIS kernels on the lamp box, which
tests/test_gpu_shade_cuts.py compares with.  These kernels share sample_li and have no oracle restatement, so the recording is the reference -- and it is one
only if it is made with the library of the commit BEFORE sample_li kept its direction (the parent of "k_shade: reuse the light sampler's direction"), built from
that commit's jet-pbrt_amd/csrc:
    JETPBRT_AMD_LIB=/path/to/parent/libjetpbrt_amd.so python tools/record_shade_cuts_parent.py [OUT.npz]
Run with this tree's own library it would record what it is meant to check.  Needs the GPU; the films are the same bits on every MI355X (fp32 arithmetic
restated operation by operation, no float atomics)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
if not os.environ.get("JETPBRT_AMD_LIB"):
    sys.exit("set JETPBRT_AMD_LIB to the parent commit's library (see the docstring)")
import jet_pbrt_amd as jp
import test_gpu_shade_cuts as T

out = {}
for name, mode, est in T.recorded_cases():
    c = jp.Context(0)
    film, cnt = T.recorded_render(c, mode, est)
    c.close()
    out[name + "_film"] = film.view(np.uint32)
    out[name + "_counters"] = cnt
    print(name, "mean %.4f" % film.mean(), cnt.tolist())
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "shade_cuts_parent.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes; library", jp.HIP_LIB_PATH)
