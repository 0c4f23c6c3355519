#!/usr/bin/env python3
"""What the pooled closest-hit pass (flat_prims_pool, csrc/jp_device.h; DESIGN.md section 5, "Pooled closest hits") has to beat, counted on the CPU on the
ray sets of tools/flat_stats.py (camera rays of the Cornell box, their first and second bounce), 64 consecutive rays a wave.  The candidate masks and the
primitive tests are the float32 models of tests/test_extend_pool_host.py on the tables the upload would copy.  Per wave:
  trips        of today's loop (flat_prims): the largest popcount of the wave's masks
  hot trips    trips in which at least one lane passes the interval test under ITS shrinking tmax (the wave then pays the inside test)
  pairs        (ray, candidate) pairs of the wave: what the list holds
  inf pairs    pairs that pass the interval test against the ORIGINAL tmax = +inf (the pooled pass runs the inside test on these lanes)
  rounds       dense rounds: ceil(pairs / 64); hot rounds: the ones in which any pair passes the interval test (nearly all)
CPU only:  python tools/extend_pool_stats.py [rays per set]"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, REPO)
import harness as H
import jet_pbrt_amd as jp
import test_extend_pool_host as M

F = np.float32


def ray_sets(sp, n, W):
    rng = np.random.default_rng(3)
    L = H.oracle_lib(); oh = L.jp_oracle_scene_new(sp)
    pxy = (np.stack([np.arange(n) % W, (np.arange(n) // W) % W], 1) + rng.random((n, 2))).astype(F)      # pixel order, as k_raygen queues them
    o = np.zeros((n, 3), F); d = np.zeros((n, 3), F)
    L.jp_oracle_camera_rays(oh, n, H.ptr(pxy), H.ptr(o), H.ptr(d))

    def otrace(o, d):
        m = o.shape[0]
        tmin = np.full(m, 0.001, F); tmax = np.full(m, np.inf, F)
        hit = np.zeros(m, np.int32); t = np.zeros(m, F); prim = np.zeros(m, np.int32); nrm = np.zeros((m, 3), F); pos = np.zeros((m, 3), F)
        L.jp_oracle_trace(oh, m, H.ptr(o), H.ptr(d), H.ptr(tmin), H.ptr(tmax), H.ptr(hit), H.ptr(t), H.ptr(prim), H.ptr(nrm), H.ptr(pos))
        return hit > 0, pos, nrm

    def bounce(pos, nrm, din):
        dd = rng.normal(size=pos.shape).astype(F); dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        return np.where(((dd * nrm).sum(1) * (-(din * nrm).sum(1)) < 0)[:, None], -dd, dd).astype(F)
    sets = [("camera", o, d)]
    for k in (1, 2):
        hit, pos, nrm = otrace(o, d)
        o, d = pos[hit], bounce(pos[hit], nrm[hit], d[hit])
        sets.append(("bounce %d" % k, o, d))
    return sets


def wave_stats(flat, prims, o, d):
    n = (len(o) // 64) * 64
    o, d = o[:n], d[:n]
    tmin = np.full(n, 0.001, F); inf = np.full(n, np.inf, F)
    with np.errstate(all="ignore"):
        mask = M.box_masks(flat, o, d, tmin, inf)
        pop = np.array([bin(int(x)).count("1") for x in mask])
        # today's loop, trip by trip: which lanes pass the interval test under the shrinking tmax
        m = mask.copy(); tmax = inf.copy(); hot = np.zeros((n // 64, 33), bool); lane_in = 0; trip = 0
        while m.any():
            idx = np.nonzero(m)[0]
            bit, p = M.lowest(m[idx]); m[idx] &= ~bit
            rec = prims[p]
            dist = (M.dot(rec[:, 12:15], rec[:, 0:3] - o[idx]) / M.dot(rec[:, 12:15], d[idx])).astype(F)
            ok = (dist > tmin[idx]) & (dist < tmax[idx])
            acc, _ = M.accept(rec, o[idx], d[idx], tmin[idx], tmax[idx])
            tmax[idx[acc]] = dist[acc]
            hot[idx[ok] // 64, trip] = True; lane_in += int(ok.sum()); trip += 1
        # the pooled pass: every pair against +inf
        inf_pairs = np.zeros(n, np.int64)
        for p in range(len(prims)):
            idx = np.nonzero(mask & (np.uint32(1) << np.uint32(p)))[0]
            rec = prims[np.full(len(idx), p)]
            dist = (M.dot(rec[:, 12:15], rec[:, 0:3] - o[idx]) / M.dot(rec[:, 12:15], d[idx])).astype(F)
            inf_pairs[idx] += (dist > tmin[idx]) & (dist < np.inf)
    w = pop.reshape(-1, 64)
    pairs = w.sum(1)
    return dict(waves=len(w), cand=pop.mean(), trips=w.max(1).mean(), hot_trips=hot.sum(1).mean(), lane_inside=lane_in / len(w), pairs=pairs.mean(), pairs_max=pairs.max(),
                inf_pairs=inf_pairs.reshape(-1, 64).sum(1).mean(), rounds=np.ceil(pairs / 64.0).mean(), util=pop.mean() / w.max(1).mean(),
                round_fill=pairs.mean() / (64.0 * np.ceil(pairs / 64.0).mean()))


def main(n=20480):
    W = 64
    be = H.scenes.build_cornell(H.scenes.HostBackend("cornell"), W, W, lambert_only=False)
    sp = be.flatten()
    flat = jp.copy_upload_table(sp, "flat").view(F).reshape(-1, 8).copy()
    prims = jp.copy_upload_table(sp, "prims").view(F).reshape(-1, 16).copy()
    print("Cornell box: %d leaves, %d primitives; 64 consecutive rays a wave" % (len(flat), len(prims)))
    print("%-9s %6s | %9s %6s %9s %11s | %7s %9s %7s %10s | %5s" % ("set", "waves", "cand/ray", "trips", "hot trips", "inside/wave", "pairs", "inf pairs", "rounds", "round fill", "util"))
    rows = []
    for name, o, d in ray_sets(sp, n, W):
        s = wave_stats(flat, prims, o, d); rows.append((name, s))
        print("%-9s %6d | %9.2f %6.2f %9.2f %11.1f | %7.1f %9.1f %7.2f %10.2f | %5.2f" % (name, s["waves"], s["cand"], s["trips"], s["hot_trips"], s["lane_inside"], s["pairs"], s["inf_pairs"], s["rounds"],
                                                                                     s["round_fill"], s["util"]))
    print("(trips / hot trips: today's loop per wave; inside/wave: lanes that run its inside test, summed over the trips; pairs / inf pairs / rounds: the pooled pass per wave;")
    print(" round fill: pairs / (64 x rounds); util: candidates per ray / trips, the lane utilisation of today's loop)")
    return rows


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
