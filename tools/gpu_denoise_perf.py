#!/usr/bin/env python3
"""Device time of the denoiser and of the guide pass (DESIGN.md "Denoiser").  GPU:
    python tools/gpu_denoise_perf.py [--reps 20] [--out FILE]
  * jp_denoise_device, 5 iterations, at 512 x 512, 1024 x 1024 and 1920 x 1080: HIP-event time of the six launches (jp_get_denoise_info), median and
    minimum over --reps runs after 3 warm-up runs; bytes moved per iteration by construction (a pixel's own two records read once, its colour
    record written: 48 B per pixel; the 24 other taps are re-reads that caches serve) and that traffic as a fraction of the HBM figure of DESIGN.md section 6
  * jp_render_guides_device at guide_spp 8 on the full-material Cornell box (512 x 512) and the bunny scene (800 x 600), next to jp_render_device of
    the same frame at 50 spp.
Every step runs in a child process under its own time limit; the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_GBS = 8000.0           # peak HBM3E bandwidth of one MI355X, the figure DESIGN.md section 6 measures against
STEPS = ["denoise:512x512", "denoise:1024x1024", "denoise:1920x1080", "guides:cornell", "guides:bunny"]


def step_denoise(w, h, reps):
    import torch
    import jet_pbrt_amd as jp
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import denoise_ref as R
    film, albedo, normal, depth = R.filter_inputs(h, w, 5)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(x).to(dev) for x in (film, albedo, normal, depth)]
    out = torch.zeros_like(t[0])
    torch.cuda.synchronize()
    ctx = jp.Context(0)
    ms = []
    for r in range(3 + reps):
        ctx.denoise_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(), sync=True, iterations=5)
        if r >= 3:
            ms.append(ctx.denoise_info().denoise_ms)
    ms = np.array(ms)
    per_it = 48.0 * w * h
    med = float(np.median(ms))
    print("denoise %4d x %4d  5 iterations  median %.3f ms  min %.3f ms  (%.3f ms / launch of 6)  %.1f MB / iteration by construction -> %.0f GB/s = %.1f %% of %.0f GB/s HBM"
          % (w, h, med, ms.min(), med / 6, per_it / 1e6, 5 * per_it / (med * 1e-3) / 1e9, 100 * 5 * per_it / (med * 1e-3) / 1e9 / HBM_GBS, HBM_GBS), flush=True)
    ctx.close()


def step_guides(scene, reps):
    import torch
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    w, h = (512, 512) if scene == "cornell" else (800, 600)
    be = scenes.build_cornell(scenes.HostBackend("perf"), w, h, lambert_only=False) if scene == "cornell" else scenes.build_bunny(scenes.HostBackend("perf"), w, h)
    dev = torch.device("cuda:0")
    film = torch.zeros((h, w, 3), dtype=torch.float32, device=dev); alb = torch.zeros_like(film); nrm = torch.zeros_like(film)
    dep = torch.zeros((h, w), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx = jp.Context(0)
    ctx.upload(be.flatten())
    rp = jp.render_params(w, h, 50, 5, 1234)
    g, r = [], []
    for k in range(2 + reps):
        ctx.render_guides_device(rp, 8, alb.data_ptr(), nrm.data_ptr(), dep.data_ptr(), sync=True)
        gm = ctx.denoise_info().guides_ms
        ctx.render_device(rp, film.data_ptr(), sync=True)
        rm = ctx.counters().render_ms
        if k >= 2:
            g.append(gm); r.append(rm)
    g, r = np.array(g), np.array(r)
    print("guides  %-7s %4d x %4d  guide_spp 8  median %.3f ms  min %.3f ms   |   render 50 spp  median %.3f ms  min %.3f ms   |   guides / render %.3f"
          % (scene, w, h, np.median(g), g.min(), np.median(r), r.min(), np.median(g) / np.median(r)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.step:
        kind, arg = a.step.split(":")
        if kind == "denoise":
            w, h = (int(v) for v in arg.split("x"))
            step_denoise(w, h, a.reps)
        else:
            step_guides(arg, a.reps)
        return 0
    for s in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            print("step %s exceeded its time limit; stopping" % s)
            return 1
        sys.stdout.write(r.stdout); sys.stdout.flush()
        if a.out:
            open(a.out, "a").write(r.stdout)
        if r.returncode != 0:
            print("step %s failed with status %d; stopping" % (s, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
