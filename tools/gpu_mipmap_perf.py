#!/usr/bin/env python3
"""The side kernel's time per frame with and without mip maps (jp_set_profiling; JpTextureMipmapInfo.texel_ms / JpTexSamplingInfo.texel_ms: the launches of
k_texel_s or k_texel_m of one render, HIP events) on two scenes of one 1024 x 1024 image under a REPEAT + BILINEAR record:
  minified floor   the image tiled 64 x 64 over a floor seen at a grazing angle: hundreds of texels under a pixel
  magnified wall   the image once over a wall that fills the frame: a texel is several pixels wide, rho <= 1 almost everywhere
Each case: one warm-up render, then --reps renders; the minimum, the median and the maximum are printed (DESIGN.md §10 "Mip maps").  GPU:
    python tools/gpu_mipmap_perf.py [--size 512] [--spp 64] [--reps 5]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jet_pbrt_amd as jp  # noqa: E402
from jet_pbrt_amd import scenes  # noqa: E402


def floor_scene(W, H, img):
    be = scenes.HostBackend("mip_perf_floor")
    be.camera((0, 3, 0), scenes._normalize(np.array([0, -0.12, -1], np.float32)), (0, 1, 0), 50.0, W, H)
    be.envlight((1, 1, 1))
    s = jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_REPEAT, jp.JP_FILTER_BILINEAR, (64, 64))
    be.rect(scenes.AXIS_XZ, -400, 400, -800, 0, 0, False, be.mat_matte(tex=be.texture_image(img, sampling=s)), None)
    be.preprocess()
    return be


def wall_scene(W, H, img):
    be = scenes.HostBackend("mip_perf_wall")
    be.camera((0, 0, 2), (0, 0, -1), (0, 1, 0), 50.0, W, H)
    be.envlight((1, 1, 1))
    s = jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_REPEAT, jp.JP_FILTER_BILINEAR, (0.125, 0.125))
    be.rect(scenes.AXIS_XY, -10, 10, -10, 10, 0, False, be.mat_matte(tex=be.texture_image(img, sampling=s)), None)
    be.preprocess()
    return be


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    W = H = a.size
    img = np.random.default_rng(1).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    ctx = jp.Context(0)
    ctx.set_profiling(True)
    mip_api = hasattr(ctx, "set_texture_mipmaps")                       # (the same script runs on a build without mip maps: k_texel_s alone)
    for name, build in (("minified floor", floor_scene), ("magnified wall", wall_scene)):
        be = build(W, H, img)
        for mip in ((False, True) if mip_api else (False,)):
            ctx.set_texture_sampling(be.flatten_texture_sampling())
            if mip_api:
                ctx.set_texture_mipmaps(jp.texture_mipmaps([1], 1.0, 0.125) if mip else None)
            ctx.upload(be.flatten(), be.flatten_textures())
            p = jp.render_params(W, H, a.spp, 5, 1234)
            ctx.render(p)                                                # warm-up
            ms, rate = [], []
            for _ in range(a.reps):
                ctx.render(p)
                ms.append(ctx.texture_sampling_info().texel_ms)
                c = ctx.counters()
                rate.append(c.samples / (c.render_ms * 1e3))
            ran = (ctx.texture_mipmap_info().mip_last_render if mip_api else 0)
            print("%-15s %-9s texel_ms min %.3f median %.3f max %.3f   %8.1f Msamples/s (median)   mip_last_render %d"
                  % (name, "k_texel_m" if mip else "k_texel_s", min(ms), float(np.median(ms)), max(ms), float(np.median(rate)), ran), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
