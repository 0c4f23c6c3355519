"""k_shade's two cuts ("k_shade: the sampler's direction, the one-sweep partition"): sample_li keeps the direction it normalised for the pdf
(every area light on a triangle, rectangle or disk, in every kernel that samples lights), and the lean sorted instance splits its region into matte and metal in one
sweep and leaves the paths that hit nothing out of the list.  Neither may change a bit of a film or a ray count: every scene is rendered with the generic kernels
(JpOptions.reserved[0] = 1: the two-sweep partition) and with the plan's choice, at one lane and at the default lane count, and compared with the oracle; the two
estimators without an oracle restatement of their own are compared with a recording of the commit before the cuts."""
import ctypes as C
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_cuts_parent.npz")


@pytest.fixture(scope="module")
def ctx():
    c = jp.Context(0)
    yield c
    c.close()


def _reserved(generic):
    return (C.c_int32 * 8)(1 if generic else 0)


def _counts(c):
    return (c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded)


def _render(ctx, params, generic, lanes, **opt):
    """lanes 0: the default lane count"""
    ctx.set_options(lanes=lanes, reserved=_reserved(generic), **opt)
    try:
        film = ctx.render(params)
        c = ctx.counters()
    finally:
        ctx.set_options()
    return film, _counts(c)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _both_ways(ctx, be, params, lit=True, **opt):
    """the scene's film with the generic kernels and with the ones the plan picks, at one lane and at the default lane count: all four the same
    bits and the same ray counts; returns that film and those counts.  lit: whether the film must be bright (None: a few rows or the light alone, not asked)"""
    ctx.upload(be.flatten())
    film0, cnt0 = _render(ctx, params, True, 1, **opt)
    assert np.isfinite(film0).all() and (lit is None or (film0.mean() > 0.02) == lit)
    for generic, lanes in ((False, 1), (True, 0), (False, 0)):
        film, cnt = _render(ctx, params, generic, lanes, **opt)
        assert _same(film, film0), "generic=%d lanes=%d: %d pixels differ" % (generic, lanes, (film != film0).any(-1).sum())
        assert cnt == cnt0, (generic, lanes, cnt, cnt0)
    return film0, cnt0


def _against_oracle(H, be, params, film, cnt):
    ref, rc = H.oracle_render(be.flatten(), params, 4)
    assert _same(film, ref), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()
    assert cnt == _counts(rc), (cnt, _counts(rc))


def _cornell(W, Hh, tallbox="metal", others="matte", lookat=(278, 273, 0), extras=None):
    """build_cornell's call sequence (main.cc:13-62) with the materials of the tall box and of the other meshes, and the camera's target, chosen"""
    be = scenes.HostBackend("shade_cuts")
    lookfrom = np.array([278, 273, 960], np.float32); front = np.array(lookat, np.float32) - lookfrom
    be.camera(lookfrom, (front / np.linalg.norm(front)).astype(np.float32), (0, 1, 0), 60.0, W, Hh)
    be.envlight((0.0, 0.0, 0.0))
    red = be.mat_matte((0.63, 0.065, 0.05)); green = be.mat_matte((0.14, 0.45, 0.091)); white = be.mat_matte((0.725, 0.71, 0.68))
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    m = (lambda matte: golden) if others == "metal" else (lambda matte: matte)
    A = scenes.cornell_assets()
    be.mesh(A["light"], True, True, mat=mat_light, radiance=scenes.light_radiance())
    be.mesh(A["floor"], True, True, mat=m(white))
    be.mesh(A["shortbox"], True, True, mat=m(white))
    be.mesh(A["tallbox"], True, True, mat=(golden if tallbox == "metal" else white))
    be.mesh(A["left"], True, True, mat=m(red))
    be.mesh(A["right"], True, True, mat=m(green))
    if extras:
        extras(be, white)
    be.preprocess()
    return be


# ---- the sorted lean instance: region sizes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell64(H):
    """the Cornell box with full materials at 64 x 64 x 16, depth 5, and the oracle's film and counts of it (computed once, never written to)"""
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    p = jp.render_params(64, 64, 16, 5, 1234)
    ref, rc = H.oracle_render(be.flatten(), p, 4)
    ref.setflags(write=False)
    return be, p, ref, _counts(rc)


def test_cornell_lean_equals_generic_equals_oracle(ctx, cornell64):
    be, p, ref, rcnt = cornell64
    film, cnt = _both_ways(ctx, be, p)
    assert _same(film, ref), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()
    assert cnt == rcnt


def test_small_batches_regions_of_256_and_fewer(ctx, cornell64):
    """max_slots = one sample per pixel a batch: 16 regions that start a batch with 256 paths (four full chunks) and hold fewer at every later bounce, down to
    partial chunks and short segments at depth 5"""
    be, p, ref, rcnt = cornell64
    film, cnt = _both_ways(ctx, be, p, max_slots=64 * 64)
    assert _same(film, ref) and cnt == rcnt


@pytest.mark.parametrize("rows,index", [(1, 3), (1, 40), (2, 20), (3, 9)])
def test_one_region_of_64_128_192(H, ctx, cornell64, rows, index):
    """a shard of one, two or three image rows rendered one sample per pixel a batch: ONE region that starts with exactly 64 (one full chunk and nothing else),
    128 or 192 paths and holds fewer than 64 in its last bounces: a row near the image's edge (walls) and rows across the boxes"""
    be, p0, _, _ = cornell64
    p = jp.render_params(64, 64, 16, 5, 1234, band_rows=rows, shard_index=index, shard_count=64 // rows)
    film, cnt = _both_ways(ctx, be, p, lit=None, max_slots=64 * rows)
    assert film.any()
    _against_oracle(H, be, p, film, cnt)


@pytest.mark.parametrize("spp", [100, 512])
def test_large_regions_lean_equals_generic(ctx, cornell64, spp):
    """regions of 1792 paths (seven passes: one group of the sweep, partly beyond the region) and of 8192 = JP_SHADE_TILE (32 passes: four groups, the 16-bit
    positions and fill counts at their largest); the generic kernels are the reference here"""
    be, _, _, _ = cornell64
    _both_ways(ctx, be, jp.render_params(64, 64, spp, 5, 1234))


# ---- classes present / absent ------------------------------------------------------------------------------------------------------------
def test_all_meshes_metal(H, ctx):
    """every mesh but the light's own is metal: the front segment holds the few paths that hit the light"""
    be = _cornell(32, 32, others="metal")
    p = jp.render_params(32, 32, 8, 5, 1234)
    film, cnt = _both_ways(ctx, be, p)
    _against_oracle(H, be, p, film, cnt)


def test_lambert_only_is_the_unsorted_instance(H, ctx):
    be = scenes.build_cornell(scenes.HostBackend("cornell_lambert"), 32, 32, lambert_only=True)
    p = jp.render_params(32, 32, 8, 5, 1234)
    film, cnt = _both_ways(ctx, be, p)
    _against_oracle(H, be, p, film, cnt)


def test_camera_sees_nothing(H, ctx):
    """the camera looks away from the box: every region holds misses only, the list is empty, the film is black and nothing waits for a chunk"""
    be = _cornell(8, 8, lookat=(278, 273, 2000))
    p = jp.render_params(8, 8, 1, 5, 1234)
    film, cnt = _both_ways(ctx, be, p, lit=False)
    assert not film.any() and cnt[1] == 0 and cnt[2] == 0
    _against_oracle(H, be, p, film, cnt)


@pytest.mark.parametrize("depth", [0, 1])
def test_depth_0_and_1(H, ctx, depth):
    """depth 0: the emission-only pass; depth 1: the first next-event estimation and nothing after it"""
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 32, 32, lambert_only=False)
    p = jp.render_params(32, 32, 4, depth, 1234)
    film, cnt = _both_ways(ctx, be, p, lit=None)
    assert film.any()
    _against_oracle(H, be, p, film, cnt)


# ---- light shapes: the direction sample_li keeps, and the branches that keep normalize --------------------------------------------------------
def _lamp_box(W, Hh):
    return scenes.build_lamp_box(scenes.HostBackend("lamp_rect"), W, Hh, scenes.lamp_rect(), full_materials=True)


def _sphere_light(center, radius, radiance):
    return lambda W, Hh: _cornell(W, Hh, extras=lambda be, white: be.sphere(center, radius, white, np.array(radiance, np.float32)))


LIGHTS = {
    "rectangle": _lamp_box,
    "disk": lambda W, Hh: scenes.build_disks(scenes.HostBackend("disks"), W, Hh),
    "sphere_from_outside": _sphere_light((150.0, 330.0, -250.0), 60.0, (20.0, 16.0, 12.0)),        # cone sampling: every shading point is outside
    "sphere_from_inside": _sphere_light((278.0, 273.0, 200.0), 1100.0, (2.0, 2.0, 2.0)),            # the camera and the whole box are inside it
    "point_direction_environment": lambda W, Hh: scenes.build_lights(scenes.HostBackend("lights"), W, Hh),
    "misc": lambda W, Hh: scenes.build_misc(scenes.HostBackend("misc"), W, Hh),                      # sphere light, null material, environment
}


@pytest.mark.parametrize("name", sorted(LIGHTS))
def test_light_shapes_against_the_oracle(H, ctx, name):
    be = LIGHTS[name](32, 32)
    p = jp.render_params(32, 32, 8, 5, 1234)
    film, cnt = _both_ways(ctx, be, p)
    _against_oracle(H, be, p, film, cnt)


# ---- the estimators that share sample_li and have no oracle restatement: the parent commit's films ------------------------------------------------
def recorded_cases():
    """(name, light sampling, estimator) of the recording; tools/record_shade_cuts_parent.py renders the same with the parent commit's library"""
    return (("power_one", "power", None), ("mis", "power", "mis"))


def recorded_render(c, mode, est):
    """the lamp box (two rectangle lights and a 64-triangle emissive mesh, metal tall box) at 32 x 32 x 8, depth 5, on a context of its own"""
    be = scenes.build_lamp_box(scenes.HostBackend("lamp_66"), 32, 32, scenes.lamp_66, full_materials=True)
    c.set_light_sampling(mode)
    c.upload(be.flatten())
    c.set_estimator(est)
    film = c.render(jp.render_params(32, 32, 8, 5, 1234))
    return film, np.array(_counts(c.counters()), np.int64)


@pytest.mark.parametrize("name,mode,est", recorded_cases())
def test_pick_and_mis_kernels_equal_the_parent_commit(name, mode, est):
    want = np.load(GOLDEN)
    c = jp.Context(0)
    try:
        film, cnt = recorded_render(c, mode, est)
    finally:
        c.close()
    assert film.mean() > 0.02
    assert np.array_equal(film.view(np.uint32), want[name + "_film"]), "%d pixels differ from the parent commit's film" % (film.view(np.uint32) != want[name + "_film"]).any(-1).sum()
    assert np.array_equal(cnt, want[name + "_counters"]), (cnt, want[name + "_counters"])
