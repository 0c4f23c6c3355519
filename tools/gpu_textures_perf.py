#!/usr/bin/env python3
"""Msamples/s of the full-material Cornell box (scenes.build_textured_cornell: metal tall box, mirror and plastic spheres), 512 x 512 x 1024 spp,
max_depth 5: untextured, then with textured walls (a 1024 x 1024 image on the back wall, a checker on the red wall).  GPU:
    python tools/gpu_textures_perf.py [--spp 1024] [--reps 3]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jet_pbrt_amd as jp  # noqa: E402
from jet_pbrt_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    W = H = a.size
    img = np.random.default_rng(1).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    cases = [("untextured", {}),
             ("textured (1024^2 image back wall, checker red wall)", dict(back=lambda b: b.texture_image(img), left=lambda b: b.texture_checker((0.63, 0.065, 0.05), (0.9, 0.8, 0.2))))]
    ctx = jp.Context(0)
    res = {}
    for name, kw in cases:
        be = scenes.build_textured_cornell(scenes.HostBackend("perf"), W, H, **kw)
        ctx.upload(be.flatten(), be.flatten_textures() if kw else None)
        p = jp.render_params(W, H, a.spp, 5, 1234)
        ctx.render(p)                                                    # warm-up
        best = 0.0
        for _ in range(a.reps):
            ctx.render(p)
            c = ctx.counters()
            best = max(best, c.samples / (c.render_ms * 1e3))
        res[name] = best
        print("%-55s %9.1f Msamples/s  (textured_last_render %d)" % (name, best, ctx.texture_info().textured_last_render), flush=True)
    v = list(res.values())
    print("textured / untextured: %.3f" % (v[1] / v[0]))
    ctx.close()


if __name__ == "__main__":
    main()
