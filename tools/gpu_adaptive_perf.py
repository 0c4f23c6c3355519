"""Adaptive sampling: the measurements of DESIGN.md "Adaptive sampling" on one GPU.  From the repository root:  python tools/gpu_adaptive_perf.py [--reps 5]
1. the headline frame (Cornell box, full materials, 512 x 512, 1024 spp): jp_render_adaptive with min = max = spp (the list twins with nothing to skip, one lane)
   against jp_render_variance at the same spp, alternating, render_ms of each frame, median and span;
2. for a few thresholds (max = spp, --min-spp 16, --step 16, dilate 1): total samples, wall time, and the mean squared error against an 8192-spp film, next to the uniform
   jp_render of (nearly) equal wall time;
3. with profiling: the kernel time of the selection (k_adapt_select, its scan and its compaction) per test, and of k_resolve_list."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jet_pbrt_amd as jp            # noqa: E402
from jet_pbrt_amd import scenes     # noqa: E402


def med_span(v, fmt="%.2f"):
    v = sorted(v)
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--thresholds", default="0.02,0.05,0.1")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--skip-uniform-case", action="store_true", help="parts 2 and 3 only")
    a = ap.parse_args()
    W = H = a.size
    ctx = jp.Context(0)
    be = scenes.build_cornell(scenes.HostBackend("adaptive_perf"), W, H, lambert_only=False)
    ctx.upload(be.flatten())
    ctx.set_film(1)
    rp = jp.render_params(W, H, a.spp, 5, 1234)

    def timed(fn):
        t0 = time.perf_counter(); out = fn(); wall = (time.perf_counter() - t0) * 1e3
        return out, wall, ctx.counters()

    # 1. nothing to skip
    uni = jp.adaptive(0.0, a.spp, 16, a.spp, 0.0, 1)
    for _ in range(0 if a.skip_uniform_case else 2):
        ctx.render_variance(rp); ctx.render_adaptive(rp, uni)
    t_var, t_ad = [], []
    for _ in range(0 if a.skip_uniform_case else a.reps):
        _, _, c = timed(lambda: ctx.render_variance(rp)); t_var.append(c.render_ms); lanes = ctx.build_info().lanes_last_render
        _, _, c = timed(lambda: ctx.render_adaptive(rp, uni)); t_ad.append(c.render_ms)
    if not a.skip_uniform_case:
        print("1. %dx%d %d spp, render_ms median (min .. max) of %d alternating frames: jp_render_variance %s (lanes %d), jp_render_adaptive min = max %s (one lane)"
              % (W, H, a.spp, a.reps, med_span(t_var), lanes, med_span(t_ad)))
        ctx.set_options(lanes=1)
        t_one = []
        for _ in range(a.reps):
            _, _, c = timed(lambda: ctx.render_variance(rp)); t_one.append(c.render_ms)
        ctx.set_options()
        print("   jp_render_variance forced onto one lane: %s" % med_span(t_one))

    # 2. thresholds
    ref = ctx.render(jp.render_params(W, H, a.ref_spp, 5, 4321)).astype(np.float64)
    for thr in [float(x) for x in a.thresholds.split(",")]:
        ad = jp.adaptive(thr, a.min_spp, a.step, a.spp, 0.0, 1)
        ctx.render_adaptive(rp, ad)
        walls, rms = [], []
        for _ in range(a.reps):
            (film, counts, _), wall, c = timed(lambda: ctx.render_adaptive(rp, ad)); walls.append(wall); rms.append(c.render_ms)
        info = ctx.adaptive_info()
        mse_a = float(((film - ref) ** 2).mean())
        mean = float(counts.mean())
        # the uniform render of equal wall time: search the spp whose median wall time is nearest
        best = None
        for spp in sorted(set(max(2, int(round(mean * f))) for f in (0.8, 0.9, 1.0, 1.1, 1.2, 1.35, 1.5))):
            p = jp.render_params(W, H, spp, 5, 1234)
            ctx.render(p)
            w = sorted(timed(lambda: ctx.render(p))[1] for _ in range(a.reps))[a.reps // 2]
            if best is None or abs(w - sorted(walls)[a.reps // 2]) < abs(best[1] - sorted(walls)[a.reps // 2]):
                best = (spp, w, float(((ctx.render(p) - ref) ** 2).mean()))
        eq = jp.render_params(W, H, int(round(mean)), 5, 1234)
        mse_eq = float(((ctx.render(eq) - ref) ** 2).mean())
        print("2. threshold %g: %d passes, %.1f Msamples (mean %.1f spp, %.1f %% of the pixels at max), wall ms %s, render_ms %s, mse %.4e | uniform %d spp (equal samples) mse %.4e ratio %.3f"
              " | uniform %d spp (wall %.2f ms, nearest in time) mse %.4e ratio %.3f"
              % (thr, info.passes, info.samples_traced / 1e6, mean, 100.0 * (counts == a.spp).mean(), med_span(walls), med_span(rms), mse_a, int(round(mean)), mse_eq, mse_a / mse_eq,
                 best[0], best[1], best[2], mse_a / best[2]))

    # 3. the selection's kernels
    ctx.set_profiling(True)
    ad = jp.adaptive(0.05, a.min_spp, a.step, a.spp, 0.0, 1)
    sel, res = [], []
    for _ in range(a.reps):
        _, counts, _ = ctx.render_adaptive(rp, ad)
        i = ctx.adaptive_info()
        tests = i.passes - 1 if (counts == a.spp).any() else i.passes       # (no test follows the pass that reaches max_spp)
        sel.append(i.select_ms / max(1, tests)); res.append(i.resolve_ms / max(1, i.passes))
    print("3. %dx%d, threshold 0.05: k_adapt_select + scan + compact %s ms per test (%d tests), k_resolve_list %s ms per pass; state %.1f MB"
          % (W, H, med_span(sel, "%.4f"), tests, med_span(res, "%.4f"), i.state_bytes_device / 1e6))
    ctx.set_profiling(False)
    ctx.close()


if __name__ == "__main__":
    main()
