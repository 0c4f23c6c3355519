#!/usr/bin/env python3
"""What an environment map costs and what its importance sampling buys (DESIGN.md "Environment maps").  GPU:
    python tools/gpu_envmap_perf.py [--reps 3] [--spp 32] [--out profiles/envmap_perf.txt]
On the bunny scene (scenes.build_bunny: four 70k-triangle meshes, a rectangle light, the environment light) at 800 x 600, equal spp, JP_LIGHTS_POWER_ONE:
  (a) the constant environment light -- k_shade_pick, the path that exists without a map
  (b) a 32 x 16 map   (c) a 1024 x 512 map   (d) a 4096 x 2048 map -- k_shade_env; the same procedural sun-and-sky at each size
per case render_ms and shade_ms (HIP-event times, JpCounters; shade_ms from a profiled run of its own), their ratios to (a), the wall time of the
upload and JpEnvInfo.table_bytes_device.  Then, at 400 x 300 under the 1024 x 512 map:
  (e) equal time: mean per-pixel L2 (pixels below 0.99 in both films) to a 2048-spp film of importance on at --spp against importance off (uniform solid
      angle, JpEnvMap.importance = -1) at the spp that takes the same device time.
Medians over --reps runs after one warm-up.  Every step runs in a child process under its own time limit; the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 800, 600
SIZES = {"a": None, "b": (32, 16), "c": (1024, 512), "d": (4096, 2048)}
STEPS = ["a", "b", "c", "d", "e"]


def sun_and_sky(w, h):
    """lat-long map, up = the map's axis: a blue gradient above the horizon, dark ground below, a sun of 1 degree radius 40 degrees up"""
    th = (np.arange(h) + 0.5) / h * np.pi; ph = (np.arange(w) + 0.5) / w * 2.0 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1)
    up = np.clip(d[..., 2], 0.0, 1.0)
    sky = np.where(d[..., 2:3] > 0, np.array([0.25, 0.45, 0.9]) * (0.35 + 0.65 * up[..., None]), np.array([0.08, 0.07, 0.06]))
    s = np.array([np.cos(np.radians(40.0)) * np.cos(1.0), np.cos(np.radians(40.0)) * np.sin(1.0), np.sin(np.radians(40.0))])
    sun = (d @ s) > np.cos(np.radians(max(1.0, 180.0 / h)))            # at least one texel
    sky[sun] = np.array([900.0, 800.0, 600.0]) * min(1.0, (1.0 / max(1.0, 180.0 / h)) ** 2)   # the same power at every map size
    return sky.astype(np.float32)


def _time(ctx, rp, reps):
    ms = []
    for k in range(1 + reps):
        film = ctx.render(rp)
        if k >= 1:
            ms.append(ctx.counters().render_ms)
    return float(np.median(ms)), film


def _l2(film, R):
    keep = (R < 0.99).all(-1) & (film < 0.99).all(-1)
    return float(np.sqrt(((film - R)[keep].astype(np.float64) ** 2).sum(-1)).mean())


def step_case(case, reps, spp):
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    be = scenes.build_bunny(scenes.HostBackend("perf"), W, H)
    ctx = jp.Context(0)
    size = SIZES[case]
    ctx.set_environment_map(None if size is None else sun_and_sky(*size), "y")
    ctx.set_light_sampling("power")
    t0 = time.perf_counter(); ctx.upload(be.flatten()); ctx.synchronize(); up_ms = (time.perf_counter() - t0) * 1e3
    rp = jp.render_params(W, H, spp, 5, 1234)
    t, film = _time(ctx, rp, reps)
    ctx.set_profiling(True)
    sh = []
    for k in range(1 + reps):
        ctx.render(rp)
        if k >= 1:
            sh.append(ctx.counters().shade_ms)
    i = ctx.env_info()
    print("(%s) %-12s %d x %d %d spp  render_ms %.3f  shade_ms %.3f  upload_ms %.1f  table_bytes_device %d  mapped %d  film mean %.4f"
          % (case, "constant" if size is None else "%d x %d" % size, W, H, spp, t, float(np.median(sh)), up_ms, i.table_bytes_device, i.mapped_last_render, float(film.mean())), flush=True)
    ctx.close()


def step_equal_time(reps, spp):
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    w, h = 400, 300
    be = scenes.build_bunny(scenes.HostBackend("perf"), w, h)
    sky = sun_and_sky(1024, 512)
    ctx = jp.Context(0)
    ctx.set_light_sampling("power")
    ctx.set_environment_map(sky, "y"); ctx.upload(be.flatten())
    R = ctx.render(jp.render_params(w, h, 2048, 5, 7))
    t_on, f_on = _time(ctx, jp.render_params(w, h, spp, 5, 1234), reps)
    ctx.set_environment_map(sky, "y", importance=-1); ctx.upload(be.flatten())
    t_off, _ = _time(ctx, jp.render_params(w, h, spp, 5, 1234), reps)
    spp_off = max(1, int(round(spp * t_on / t_off)))
    t_eq, f_off = _time(ctx, jp.render_params(w, h, spp_off, 5, 1234), reps)
    print("(e) equal time  1024 x 512 sun-and-sky, %d x %d: importance on %d spp %.3f ms  L2 to the 2048-spp film %.5f   |   off %d spp %.3f ms  L2 %.5f   |   L2 ratio off / on %.2f"
          % (w, h, spp, t_on, _l2(f_on, R), spp_off, t_eq, _l2(f_off, R), _l2(f_off, R) / _l2(f_on, R)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.step:
        if a.step == "e":
            step_equal_time(a.reps, a.spp)
        else:
            step_case(a.step, a.reps, a.spp)
        return 0
    for s in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps), "--spp", str(a.spp)], stdout=subprocess.PIPE, text=True, timeout=240)
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
