"""The float64 ray caster of the per-ray tests (tests/rays_ref.py) held against the fp32 CPU oracle (jp_oracle_trace), without a GPU: on every scene and ray set
of tests/rays_sets.py the oracle's hit flag equals the float64 verdict on EVERY decisive ray; the oracle's distance on decisive hit rays stays within the
figure rays_ref.py records (of which T_TOL, the GPU's tolerance, is four times); at most 2 % of the rays of any set are non-decisive; the bracket sets
are what their names say.  These pin the margin, the grazing bound and T_TOL of rays_ref.py before any GPU result is looked at."""
import time

import numpy as np
import pytest

import rays_ref as R
import rays_sets as RS


def test_reference_on_hand_made_rays():
    """the caster itself, on cases worked out by hand: each shape kind hit and missed, the far end on both sides, zero components, a tangent ray"""
    hb, sp = RS.build("all_lights")
    sh = RS.shapes("all_lights")
    # the ceiling rectangle y = 2.5 over [-2, 2]^2, the wall x = -2.5, the sphere (0.5, -0.5, 0.5) r 0.8, a disk
    o = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [3, 0, 0], [0.5, -0.5, 5], [0.5, -0.5, 5], [0.5, 0.3 - 1e-9, 5], [1.9, 0, 1.9]], np.float64)
    d = np.array([[0, 1, 0], [0, 1, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 1, 0]], np.float64)
    tmin = np.full(8, 0.001); tmax = np.array([np.inf, 2.4, np.inf, np.inf, np.inf, 3.0, np.inf, np.inf])
    with np.errstate(divide="raise", over="raise", invalid="raise"):
        r = R.cast(sh, o, d, tmin, tmax)
    kind = [int(sh.kind[p]) if p >= 0 else -1 for p in r["prim"]]
    assert kind[:6] == [R.RECTANGLE, -1, R.RECTANGLE, -1, R.SPHERE, -1]
    assert np.allclose(r["t"][[0, 2, 4]], [2.5, 2.5, 3.7])
    assert r["decisive"][:6].all() and not r["decisive"][6]              # the ray 1e-9 inside the sphere's silhouette is a close call
    assert r["hit"][7] and r["decisive"][7]                                # 0.1 from two edges of the ceiling: m is 1e-5 * S


@pytest.mark.parametrize("name", RS.SCENES)
def test_oracle_agrees_on_every_decisive_ray(name):
    hb, sp = RS.build(name)
    sh = RS.shapes(name)
    worst = {"flat": 0.0, "sphere": 0.0}
    t_cast = 0.0
    for which, (o, d, tmin, tmax) in RS.ray_sets(name).items():
        t0 = time.perf_counter()
        with np.errstate(divide="raise", over="raise", invalid="raise"):                                     # zero components and infinite far ends included: no warning
            ref = RS.reference(name, which)
        t_cast += time.perf_counter() - t0
        dec = ref["decisive"]
        share = 1.0 - dec.mean()
        ohit, ot, oprim = RS.oracle_trace(sp, o, d, tmin, tmax)
        bad = np.nonzero(dec & ((ohit != 0) != ref["hit"]))[0]
        uq = dec & ref["unique"] & (ohit != 0)
        err = np.abs(ot[uq].astype(np.float64) - ref["t"][uq]) / np.maximum(np.abs(ref["t"][uq]), sh.S)
        cls = R.shape_class(sh, ref["prim"][uq])
        for k in worst:
            worst[k] = max(worst[k], float(err[cls == k].max()) if (cls == k).any() else 0.0)
        err = np.r_[err, 0.0]
        wrong_prim = int((oprim[uq] != ref["prim"][uq]).sum())
        print("%-14s %-8s n %5d  hits %.3f  non-decisive %.4f  oracle disagrees on %d  wrong prim %d  worst dt %.3e" %
              (name, which, len(o), ref["hit"].mean(), share, len(bad), wrong_prim, err.max()))
        assert share <= R.MAX_NON_DECISIVE or not RS.capped(name, which), (name, which, share)
        assert len(bad) == 0, (name, which, bad[:8], o[bad[:8]], d[bad[:8]], tmin[bad[:8]], tmax[bad[:8]])
        assert wrong_prim == 0, (name, which)
        if which == "near":
            assert not ref["hit"][dec].any(), (name, "a bracket ray with its far end before the nearest hit is occluded")
        if which == "far":
            assert ref["hit"][dec].all(), (name, "a bracket ray with its far end behind the hit is not occluded")
    print("%-14s oracle's worst |t - t64| / max(|t|, S): flat %.3e sphere %.3e   float64 casts: %.1f s" % (name, worst["flat"], worst["sphere"], t_cast))
    for k in worst:
        assert worst[k] <= R.ORACLE_T_WORST[k], (name, k, worst[k])


def test_reference_speed():
    """20,000 rays against 3,000 triangles in a few seconds"""
    rng = np.random.default_rng(1)
    sh = R.Shapes.from_triangles(rng.uniform(-3, 3, (3000, 1, 3)) + rng.normal(0, 0.5, (3000, 3, 3)))
    o = rng.uniform(-4, 4, (20000, 3)); d = rng.normal(size=(20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0 = time.perf_counter()
    r = R.cast(sh, o, d, np.full(20000, 0.001), np.full(20000, np.inf))
    dt = time.perf_counter() - t0
    print("20,000 rays x 3,000 triangles: %.2f s, hits %.3f, decisive %.4f" % (dt, r["hit"].mean(), r["decisive"].mean()))
    assert r["hit"].mean() > 0.5 and dt < 10.0
