#!/usr/bin/env python3
"""What picking one light per bounce buys (DESIGN.md "Light selection").  GPU:
    python tools/gpu_light_pick_perf.py [--reps 5] [--out FILE]
On the 66-light box of tests/test_gpu_light_pick.py (scenes.lamp_66: two rectangle lights and a 64-triangle emissive mesh) at 256 x 256:
  (a) equal-spp:   device time of a 64-spp frame, JP_LIGHTS_ALL against JP_LIGHTS_POWER_ONE, and the shadow rays of each
  (b) equal-time:  mean per-pixel L2 (pixels below 0.99 in both films) to a 4096-spp ALL film of ALL at 16 spp against POWER_ONE at the spp that takes
                   the same device time by (a)
  (c) mesh lamp:   device time of a 64-spp frame of the box whose lamp is 4096 emissive triangles (scenes.lamp_mesh(64, 32)), POWER_ONE (ALL refuses it)
Times are HIP-event times of jp_render_device (JpCounters.render_ms), median over --reps runs after one warm-up.  Every step runs in a child process
under its own time limit; the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W = H = 256
STEPS = ["equal", "lamp4096"]


def _time(ctx, jp, rp, reps):
    ms = []
    for k in range(1 + reps):
        film = ctx.render(rp)
        if k >= 1:
            ms.append(ctx.counters().render_ms)
    return float(np.median(ms)), film, ctx.counters()


def _l2(film, R):
    keep = (R < 0.99).all(-1) & (film < 0.99).all(-1)
    return float(np.sqrt(((film - R)[keep].astype(np.float64) ** 2).sum(-1)).mean())


def step_equal(reps):
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    be = scenes.build_lamp_box(scenes.HostBackend("perf"), W, H, scenes.lamp_66)
    ctx = jp.Context(0)
    ctx.set_light_sampling(None); ctx.upload(be.flatten())
    R = ctx.render(jp.render_params(W, H, 4096, 5, 7))
    t_all, _, c_all = _time(ctx, jp, jp.render_params(W, H, 64, 5, 1234), reps)
    t_all16, f_all16, _ = _time(ctx, jp, jp.render_params(W, H, 16, 5, 1234), reps)
    ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    t_one, _, c_one = _time(ctx, jp, jp.render_params(W, H, 64, 5, 1234), reps)
    print("(a) equal spp   66 lights %d x %d  64 spp  ALL %.3f ms (%d shadow rays)  POWER_ONE %.3f ms (%d shadow rays)  time ratio %.2f  shadow-ray ratio %.2f"
          % (W, H, t_all, c_all.shadow_rays, t_one, c_one.shadow_rays, t_all / t_one, c_all.shadow_rays / max(1, c_one.shadow_rays)), flush=True)
    spp_one = max(1, int(round(t_all16 / (t_one / 64.0))))               # the POWER_ONE spp that takes the time of ALL at 16 spp
    t_eq, f_one, _ = _time(ctx, jp, jp.render_params(W, H, spp_one, 5, 1234), reps)
    print("(b) equal time  ALL 16 spp %.3f ms  L2 to the 4096-spp ALL film %.5f   |   POWER_ONE %d spp %.3f ms  L2 %.5f   |   L2 ratio %.2f"
          % (t_all16, _l2(f_all16, R), spp_one, t_eq, _l2(f_one, R), _l2(f_all16, R) / _l2(f_one, R)), flush=True)
    ctx.close()


def step_lamp(reps):
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    be = scenes.build_lamp_box(scenes.HostBackend("perf"), W, H, scenes.lamp_mesh(64, 32))
    ctx = jp.Context(0)
    ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    t, film, c = _time(ctx, jp, jp.render_params(W, H, 64, 5, 1234), reps)
    i = ctx.light_info()
    print("(c) mesh lamp   %d lights %d x %d  64 spp  POWER_ONE %.3f ms (%d shadow rays, film mean %.4f, traversal mode %d)"
          % (i.n_lights, W, H, t, c.shadow_rays, float(film.mean()), ctx.build_info().traversal_mode), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.step:
        (step_equal if a.step == "equal" else step_lamp)(a.reps)
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
