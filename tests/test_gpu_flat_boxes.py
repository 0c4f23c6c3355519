"""The box phase of the flat-shape instances (csrc/jp_device.h: flat_boxes_lean) on the GPU: k_extend<2, FeatFlat>, k_shadow<2, FeatFlat>
and k_trace_flat must give what the generic instances (JpOptions.reserved[0] = 1, flat_boxes) give, bit for bit -- films, ray counters, hit records.  The
routine accumulates its mask under the execution mask and, for closest hits, leaves out the clamp against an infinite tmax; the scenes and rays cover what
could tell the two apart: coherent camera waves and incoherent bounce waves, partly active waves (the ends of the queues), shadow rays up to the ceiling
light and down to a light on the FLOOR, whole ray groups of one direction octant, mixed groups, groups with one odd lane, axis-parallel rays (infinite
reciprocals, the NaN case of the box test), origins on the wall planes, finite far ends and far ends below tmin."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = jp.Context(0)
    yield c
    c.close()


def _reserved(generic):
    return (C.c_int32 * 8)(1 if generic else 0)


def _render(ctx, params, generic, lanes):
    """lanes 0: the default lane count"""
    ctx.set_options(lanes=lanes, reserved=_reserved(generic))
    try:
        film = ctx.render(params)
        c = ctx.counters()
    finally:
        ctx.set_options()
    return film, (c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded)


def _lean_equals_generic(ctx, be, params, lit=True):
    """lit: the film shows lit surfaces (false at maxDepth 0, where only the emitter itself is seen)"""
    ctx.upload(be.flatten())
    film0, cnt0 = _render(ctx, params, True, 1)
    assert np.isfinite(film0).all() and (film0.mean() > 0.02 if lit else film0.max() > 0)
    for generic, lanes in ((False, 1), (True, 0), (False, 0)):
        film, cnt = _render(ctx, params, generic, lanes)
        assert np.array_equal(film.view(np.uint32), film0.view(np.uint32)), "generic=%d lanes=%d: %d pixels differ" % (generic, lanes, (film != film0).any(-1).sum())
        assert cnt == cnt0, (generic, lanes, cnt, cnt0)
    return cnt0


@pytest.mark.parametrize("max_depth", [5, 0])
def test_cornell_film_and_counters(ctx, max_depth):
    """maxDepth 5: camera, bounce and shadow waves.  maxDepth 0: camera waves only"""
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    cnt = _lean_equals_generic(ctx, be, jp.render_params(64, 64, 8, max_depth, 1234), lit=max_depth > 0)
    assert cnt[0] >= 64 * 64 * 8 and cnt[1] > 0


def test_light_on_the_floor(ctx):
    """the Cornell box lit by a rectangle just above the floor that faces up: every shadow ray points down"""
    def lamp(be, m):
        x0, x1, z0, z1, _ = scenes.LAMP_RECT
        be.rect(scenes.AXIS_XZ, x0, x1, -z1, -z0, 1.0, False, m["light"], scenes.light_radiance())
    be = scenes.build_lamp_box(scenes.HostBackend("floor_light"), 64, 64, lamp, full_materials=True)
    cnt = _lean_equals_generic(ctx, be, jp.render_params(64, 64, 8, 5, 1234))
    assert cnt[2] > 64 * 64                                              # shadow rays were traced


def _trace_rays():
    """64 groups of 64 rays (k_trace_flat gives a wave 64 consecutive rays)"""
    rng = np.random.default_rng(17)
    n = 4096
    g = np.arange(n) // 64
    o = np.stack([rng.uniform(5.0, 550.0, n), rng.uniform(5.0, 540.0, n), rng.uniform(-555.0, -5.0, n)], -1).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tmin = np.full(n, 0.001, np.float32); tmax = np.full(n, np.inf, np.float32)
    octant = np.array([[1 if (k >> a) & 1 else -1 for a in range(3)] for k in range(8)], np.float32)
    one = (g < 16) | ((g >= 32) & (g < 48))                               # groups 0-15: one octant each; 16-31: mixed; 32-47: one octant with one odd lane
    d[one] = np.abs(d[one]) * octant[g[one] % 8]
    for grp in range(32, 48):
        lane, axis = int(rng.integers(0, 64)), int(rng.integers(0, 3))
        d[grp * 64 + lane, axis] = -d[grp * 64 + lane, axis] if grp % 2 else np.float32(0.0) * (-1 if grp % 4 else 1)
    ax = (g >= 48) & (g < 56)                                             # 48-55: axis-parallel rays, zeros of both signs in the other components
    k = rng.integers(0, 3, n); sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    par = np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0); par[np.arange(n), k] = sgn
    d[ax] = par[ax].astype(np.float32)
    wall = g >= 56                                                       # 56-63: origins exactly on the planes of the walls, floor, ceiling and back
    planes = [np.array([0.0, 549.6, 556.0], np.float32), np.array([0.0, 548.8], np.float32), np.array([0.0, -559.2], np.float32)]
    for i in np.nonzero(wall)[0]:
        a = int(rng.integers(0, 3)); o[i, a] = rng.choice(planes[a])
    tmax[(g % 4 == 1)] = rng.uniform(50.0, 600.0, n).astype(np.float32)[(g % 4 == 1)]       # every fourth group: a finite far end
    tmax[(g % 16 == 3) & (np.arange(n) % 7 == 0)] = np.float32(0.0005)                      # some rays with tmax < tmin
    return o, d, tmin, tmax


def test_trace_hit_records(ctx):
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    ctx.upload(be.flatten())
    o, d, tmin, tmax = _trace_rays()
    out = []
    for generic in (True, False):
        ctx.set_options(reserved=_reserved(generic))
        try:
            out.append(ctx.trace(o, d, tmin, tmax))
        finally:
            ctx.set_options()
    (h0, t0, p0, n0), (h1, t1, p1, n1) = out
    assert h0.sum() > len(o) // 2 and (h0 == 0).sum() > 16
    assert np.array_equal(h0, h1) and np.array_equal(p0, p1)
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(n0.view(np.uint32), n1.view(np.uint32))
