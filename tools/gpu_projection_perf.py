#!/usr/bin/env python3
"""The time of ray generation per camera: k_raygen<false> (the pinhole) and k_raygen_proj under each projection, on the configs[2] frame (the Cornell scene, full
materials, 512 x 512), from `rocprofv3 --kernel-trace --stats`.  One child process per camera -- the three projections share a kernel name -- each under a time
limit, one after the other; the first that fails ends the run.  Each child renders one warm-up frame and --reps frames of --spp samples (64 spp: one batch of 2^24
slots per frame, so one k_raygen launch per frame).  Prints the average time of a launch per camera (DESIGN.md §10 "Projections").  GPU:
    python tools/gpu_projection_perf.py [--size 512] [--spp 64] [--reps 5] [--out DIR]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERAS = ["perspective", "ortho", "equirect", "fisheye"]


def workload(a):
    sys.path.insert(0, ROOT)
    import jet_pbrt_amd as jp
    from jet_pbrt_amd import scenes
    be = scenes.build_cornell(scenes.HostBackend("projection_perf"), a.size, a.size, lambert_only=False)
    ctx = jp.Context(0)
    ctx.set_options(lanes=1)                                          # one lane: one k_raygen launch per batch
    ctx.upload(be.flatten())
    if a.workload != "perspective":
        ctx.set_projection(a.workload, ortho_scale=500.0 if a.workload == "ortho" else 0.0)
    p = jp.render_params(a.size, a.size, a.spp, 5, 1234)
    for _ in range(a.reps + 1):
        film = ctx.render(p)
    c = ctx.counters()
    print("%s: film mean %.4f, %.1f Msamples/s, projected_last_render %d" % (a.workload, float(film.mean()), c.samples / (c.render_ms * 1e3), ctx.projection_info().projected_last_render), flush=True)
    ctx.close()


def raygen_rows(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_raygen" in r.get("Name", ""):
                rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--workload", choices=CAMERAS, default=None, help="(internal) render under this camera instead of driving the profiler")
    a = ap.parse_args()
    if a.workload:
        return workload(a)
    out = a.out or tempfile.mkdtemp(prefix="projection_perf_")
    for cam in CAMERAS:
        d = os.path.join(out, cam)
        cmd = ["timeout", "-k", "10", "180", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--workload", cam, "--size", str(a.size), "--spp", str(a.spp), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            sys.exit("gpu_projection_perf: the %s run failed with status %d; nothing more is started" % (cam, r.returncode))
        print([l for l in r.stdout.splitlines() if l.startswith(cam + ":")][-1], flush=True)
        rows = raygen_rows(d)
        if not rows:
            sys.exit("gpu_projection_perf: no k_raygen row in the kernel statistics under %s" % d)
        for name, calls, total in rows:
            print("%-12s %-40s %3d launches, %9.1f us per launch (%d x %d x %d spp)" % (cam, name.split("(")[0][:40], calls, total / calls / 1e3, a.size, a.size, a.spp), flush=True)


if __name__ == "__main__":
    main()
