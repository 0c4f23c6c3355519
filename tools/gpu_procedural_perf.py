#!/usr/bin/env python3
"""The side kernel's time per frame with and without a procedural record (jp_set_profiling; JpTexSamplingInfo.texel_ms: the launches of k_texel or k_texel_p of
one render, HIP events) on one floor under two cameras:
  near   the camera looks down at the floor from 3 units: the cone's footprint stays below every octave's fade, all octaves are evaluated
  far    the camera looks along the floor to the horizon: the footprint swallows octave after octave and the loop ends early
Per view: the plain checker (k_texel), then each kind antialiased and point-sampled (k_texel_p).  Each case: one warm-up render, then --reps renders; the minimum,
the median and the maximum are printed (DESIGN.md §10 "Procedural textures").  GPU:
    python tools/gpu_procedural_perf.py [--size 512] [--spp 64] [--reps 5] [--octaves 8]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jet_pbrt_amd as jp  # noqa: E402
from jet_pbrt_amd import scenes  # noqa: E402

KINDS = (("fbm", jp.JP_PROC_FBM), ("turbulence", jp.JP_PROC_TURBULENCE), ("marble", jp.JP_PROC_MARBLE), ("checker", jp.JP_PROC_CHECKER_AA))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--octaves", type=int, default=8)
    a = ap.parse_args()
    W = H = a.size
    ctx = jp.Context(0)
    ctx.set_profiling(True)
    for view in ("near", "far"):
        be = scenes.build_procedural_floor(scenes.HostBackend("procedural_perf_" + view), W, H, None, view)   # (the records go to the context below: one scene per view)
        cases = [("plain checker", None)]
        for name, kind in KINDS:
            for aa in (1, -1):
                cases.append(("%s %s" % (name, "aa" if aa > 0 else "point"), jp.procedural(kind, m=(2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0), octaves=a.octaves, antialias=aa)))
        for name, rec in cases:
            ctx.set_texture_procedurals(None if rec is None else jp.texture_procedurals([rec]))
            ctx.upload(be.flatten(), be.flatten_textures())
            p = jp.render_params(W, H, a.spp, 5, 1234)
            ctx.render(p)                                                # warm-up
            ms, rate = [], []
            for _ in range(a.reps):
                ctx.render(p)
                ms.append(ctx.texture_sampling_info().texel_ms)
                c = ctx.counters()
                rate.append(c.samples / (c.render_ms * 1e3))
            print("%-5s %-18s %-9s texel_ms min %.3f median %.3f max %.3f   %8.1f Msamples/s (median)   procedural_last_render %d"
                  % (view, name, "k_texel_p" if rec is not None else "k_texel", min(ms), float(np.median(ms)), max(ms), float(np.median(rate)),
                     ctx.procedural_info().procedural_last_render), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
