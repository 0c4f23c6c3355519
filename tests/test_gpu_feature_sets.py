"""Feature sets: the tiny-scene kernels exist a second time without the code a scene of flat shapes, area lights on them
and matte / metal materials cannot reach; the upload's plan picks the instance, JpOptions.reserved[0] = 1 forces the generic kernels.  Every
scene here is rendered both ways, with one lane and with the default lane count: the films must be the same bits -- and, for the scenes that
hold something a lean instance lacks, the oracle's bits, which a wrongly chosen lean instance (black or different pixels) would not give."""
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


def _both_ways(ctx, be, params):
    """the scene's film with the generic kernels and with the ones the plan picks, at one lane and at the default lane count: all four the same
    bits and the same ray counts; returns that film"""
    ctx.upload(be.flatten())
    film0, cnt0 = _render(ctx, params, True, 1)
    assert np.isfinite(film0).all() and film0.mean() > 0.02
    for generic, lanes in ((False, 1), (True, 0), (False, 0)):
        film, cnt = _render(ctx, params, generic, lanes)
        assert np.array_equal(film.view(np.uint32), film0.view(np.uint32)), "generic=%d lanes=%d: %d pixels differ" % (generic, lanes, (film != film0).any(-1).sum())
        assert cnt == cnt0, (generic, lanes, cnt, cnt0)
    return film0


# ---- 1, 2: the scenes the lean instances exist for (sorted and unsorted k_shade) ----------------------------------------------------
@pytest.mark.parametrize("lambert_only", [False, True])
def test_cornell_lean_equals_generic(ctx, lambert_only):
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=lambert_only)
    _both_ways(ctx, be, jp.render_params(64, 64, 16, 5, 1234))


# ---- 3: one scene per axis that a lean instance must NOT get ---------------------------------------------------------------------------
def _cornell_with(shortbox=None, extras=None):
    """build_cornell's call sequence (main.cc:13-62) with the short box's material chosen by `shortbox(be)`"""
    W = Hh = 32
    be = scenes.HostBackend("cornell_axis")
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    front = lookat - lookfrom
    be.camera(lookfrom, (front / np.linalg.norm(front)).astype(np.float32), (0, 1, 0), 60.0, W, Hh)
    be.envlight((0.0, 0.0, 0.0))
    red = be.mat_matte((0.63, 0.065, 0.05)); green = be.mat_matte((0.14, 0.45, 0.091)); white = be.mat_matte((0.725, 0.71, 0.68))
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    A = scenes.cornell_assets()
    be.mesh(A["light"], True, True, mat=mat_light, radiance=scenes.light_radiance())
    be.mesh(A["floor"], True, True, mat=white)
    be.mesh(A["shortbox"], True, True, mat=(shortbox(be) if shortbox else white))
    be.mesh(A["tallbox"], True, True, mat=golden)
    be.mesh(A["left"], True, True, mat=red)
    be.mesh(A["right"], True, True, mat=green)
    if extras:
        extras(be, white)
    be.preprocess()
    return be


FALLBACK = {
    "sphere": dict(extras=lambda be, white: be.sphere((150.0, 330.0, -250.0), 60.0, white, None)),
    "point_light": dict(extras=lambda be, white: be.pointlight((278.0, 400.0, -279.0), (40000.0, 30000.0, 20000.0))),
    "glass_box": dict(shortbox=lambda be: be.mat_glass(1.5, (0.95, 0.95, 0.95), (0.9, 0.95, 0.9))),
}


@pytest.mark.parametrize("axis", sorted(FALLBACK))
def test_fallback_scene_keeps_the_needed_code(H, ctx, axis):
    be = _cornell_with(**FALLBACK[axis])
    p = jp.render_params(32, 32, 8, 5, 1234)
    film = _both_ways(ctx, be, p)
    ref, _ = H.oracle_render(be.flatten(), p, 4)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()


# ---- 4: the second lean shape / light combination: triangles and rectangles under a rectangle light -----------------------------------
def test_rectangles_and_rectangle_light(H, ctx):
    def lamp(be, m):
        scenes.lamp_rect()(be, m)
        be.rect(scenes.AXIS_XZ, 90.0, 260.0, -330.0, -160.0, 210.0, False, m["white"], None)     # a two-sided panel above the floor
        be.rect(scenes.AXIS_XY, 300.0, 480.0, 20.0, 300.0, -200.0, True, m["white"], None)       # and an upright one
    be = scenes.build_lamp_box(scenes.HostBackend("rect_box"), 32, 32, lamp, full_materials=True)
    p = jp.render_params(32, 32, 8, 5, 1234)
    film = _both_ways(ctx, be, p)
    ref, _ = H.oracle_render(be.flatten(), p, 4)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()


# ---- 5: jp_trace stays what it was: k_trace is generic, the option must not disturb it ---------------------------------------------------
def test_trace_ignores_the_option(ctx):
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    ctx.upload(be.flatten())
    rng = np.random.default_rng(11)
    n = 4096
    o = np.stack([rng.uniform(5.0, 550.0, n), rng.uniform(5.0, 540.0, n), rng.uniform(-555.0, -5.0, n)], -1).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tmin = np.full(n, 0.001, np.float32); tmax = np.full(n, np.inf, np.float32)
    out = []
    for generic in (False, True):
        ctx.set_options(reserved=_reserved(generic))
        try:
            out.append(ctx.trace(o, d, tmin, tmax))
        finally:
            ctx.set_options()
    (h0, t0, p0, _), (h1, t1, p1, _) = out
    assert h0.sum() > n // 2                                             # origins inside the box: nearly every ray hits a wall
    assert np.array_equal(h0, h1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(p0, p1)
