#!/usr/bin/env python3
"""What the MIS estimator costs per sample (DESIGN.md "Estimator").  GPU:
    python tools/gpu_mis_perf.py [--reps 3] [--out profiles/mis_perf.txt]
Msamples/s of JP_ESTIMATOR_NEE against JP_ESTIMATOR_MIS, the same upload (JP_LIGHTS_POWER_ONE), equal spp, on
  (a) the lit box: the Cornell box with matte, metal and a plastic sphere, one rectangle light and a 16 x 8 map, 512 x 512 at 64 spp
  (b) configs[2] of bench.py: the reference's Cornell scene (metal tall box) at 512 x 512, 1024 spp
Per case render_ms (HIP-event time, JpCounters; median over --reps runs after one warm-up) of each estimator and their ratio.  Every step runs in a
child process under its own time limit; the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STEPS = ["a", "b"]


def bright_map():
    """a 16 x 8 sky: a dim gradient and three bright texels"""
    m = np.zeros((8, 16, 3), np.float64)
    for r in range(8):
        m[r] = np.array([0.05, 0.07, 0.10]) * (1.0 + 0.25 * r)
    m[1, 3] = (40.0, 30.0, 20.0); m[2, 11] = (25.0, 20.0, 18.0); m[5, 7] = (30.0, 30.0, 30.0)
    return (m * 0.05).astype(np.float32)


def step(case, reps):
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    w = h = 512
    if case == "a":
        def lamp(be, m):
            scenes.lamp_rect()(be, m)
            be.envlight((0.5, 0.5, 0.5))
            be.sphere((420, 90, -120), 50.0, be.mat_plastic((0.35, 0.12, 0.48), (0.3, 0.25, 0.2), 0.05, False))
        be = scenes.build_lamp_box(scenes.HostBackend("perf"), w, h, lamp, full_materials=True)
        sky, spp, name = bright_map(), 64, "lit box, 16 x 8 map"
    else:
        be = scenes.build_cornell(scenes.HostBackend("perf"), w, h)
        sky, spp, name = None, 1024, "configs[2] (Cornell, metal tall box)"
    ctx = jp.Context(0)
    ctx.set_environment_map(sky, "y"); ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    rp = jp.render_params(w, h, spp, 5, 1234)
    ms, mean = {}, {}
    for est in ("nee", "mis"):
        ctx.set_estimator(est)
        t = []
        for k in range(1 + reps):
            film = ctx.render(rp)
            if k >= 1:
                t.append(ctx.counters().render_ms)
        assert ctx.estimator_info().mis_last_render == (1 if est == "mis" else 0)
        ms[est], mean[est] = float(np.median(t)), float(film.mean())
    n = w * h * spp / 1e6
    print("(%s) %-38s %d x %d %4d spp  NEE %8.3f ms %8.1f Msamples/s   MIS %8.3f ms %8.1f Msamples/s   MIS / NEE time %.3f   film means %.4f / %.4f"
          % (case, name, w, h, spp, ms["nee"], n / ms["nee"] * 1e3, ms["mis"], n / ms["mis"] * 1e3, ms["mis"] / ms["nee"], mean["nee"], mean["mis"]), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.reps)
        return 0
    for s in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True, timeout=180)
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
