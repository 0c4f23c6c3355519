"""k_shadow_pair (csrc/jp_kernels.hip; DESIGN.md section 5, "Shadow pairs"): the shadow kernel of the flat-shape scenes with <= 32 primitives and two or more
shadow planes traces an entry's rays two at a time.  Every verdict must be the single walk's, so every scene here is rendered with the generic kernels
(JpOptions.reserved[0] = 1) and with the ones the selector picks, at one lane and at the default lane count: the films must be the same bits and the four
ray counters equal; where the existing tests hold a scene to the oracle's bits (the Cornell box, rectangles under rectangle lights) these do too.

Scenes: the Cornell box (two triangle lights: nearly every entry holds two rays) at maxDepth 5, 1 and 0; one lamp triangle moved to the floor under the
boxes, whose tops never see it and whose side planes cut it, so that one-ray and two-ray entries mix in a wave; three area lights (an odd last ray, three planes); rectangle lights and rectangle
panels (rect_hit); and the scenes the selector must NOT give the pair kernel: one light only (one plane), 34 primitives.  test_selector_choice asserts the
kernel picked for each of them (Context.shadow_kernel).

Region fills: a region's fill cannot be read back, so the frames are chosen by what they can hold.  8 x 8 at 1 spp is one region of at most 64 entries (one
wave, partly filled), 8 x 8 at 4 spp one region of at most 256; from there up to 64 x 64 at 16 spp (256 regions of 256 slots), and the deeper bounces of a
maxDepth-5 frame leave regions with every fill from 1 upwards, across the wave boundaries at 63 / 64 / 65.  A region of more than 256 entries -- the second
trip of a thread through the entry loop, with the prefetched plane-1 direction -- needs more paths than 64 x 64 x 16 (a region grows past 256 slots only when
there are more 256-path chunks than workgroups): test_regions_beyond_one_block renders 128 x 128 at 8 spp with one workgroup per CU, i.e. 512-slot regions."""
import ctypes as C
import os

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


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _floor_lamp(be, m):
    """the Cornell lamp pulled apart: its first triangle stays under the ceiling, the second, much larger, lies just above the floor under and around the two
    boxes.  A light sample below a receiver's horizon is rejected before it becomes a ray: the tops of the boxes never see the floor triangle, and the planes of
    the boxes' sides cut it, so their points see it for some samples only -- one-ray entries next to two-ray entries in the same waves"""
    x0, x1, z0, z1 = scenes.LAMP_RECT[:4]
    d = scenes.asset_dir()
    top = os.path.join(d, "lamp_half_ceiling.obj"); low = os.path.join(d, "lamp_half_floor.obj")
    if not os.path.exists(top):
        scenes.write_obj(top, np.array([(x1, 548.7, z0), (x1, 548.7, z1), (x0, 548.7, z1)], np.float32), np.array([(0, 1, 2)]))    # cornellbox/light.obj's first triangle
    if not os.path.exists(low):
        scenes.write_obj(low, np.array([(30, 0.5, 30), (30, 0.5, 530), (530, 0.5, 30)], np.float32), np.array([(0, 1, 2)]))
    be.mesh(top, True, True, mat=m["light"], radiance=scenes.light_radiance())
    be.mesh(low, True, True, mat=m["light"], radiance=(4.0, 4.0, 4.0))


def _small_box(name, W, lamp, extras=None):
    """the Cornell box without its short box (20 primitives) and without a light: lamp(be, mats) and extras(be, mats) add the rest"""
    be = scenes.HostBackend(name)
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    front = lookat - lookfrom
    be.camera(lookfrom, (front / np.linalg.norm(front)).astype(np.float32), (0, 1, 0), 60.0, W, W)
    red = be.mat_matte((0.63, 0.065, 0.05)); green = be.mat_matte((0.14, 0.45, 0.091)); white = be.mat_matte((0.725, 0.71, 0.68))
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    m = dict(white=white, light=be.mat_matte((0.65, 0.65, 0.65)))
    A = scenes.cornell_assets(); T = scenes.cornell_textured_assets()
    lamp(be, m)
    for path, mat in ((T["floor_only"], white), (T["ceiling"], white), (T["back"], white), (A["tallbox"], golden), (A["left"], red), (A["right"], green)):
        be.mesh(path, True, True, mat=mat)
    if extras:
        extras(be, m)
    be.preprocess()
    return be


def _three_lamps(be, m):
    scenes.lamp_mesh(1, 1)(be, m)                                                                # two triangle lights on the ceiling ...
    be.rect(scenes.AXIS_XZ, 60.0, 150.0, -180.0, -110.0, 548.7, True, m["light"], (30.0, 24.0, 18.0))   # ... and a rectangle light next to them


def _two_rect_lamps(be, m):
    be.rect(scenes.AXIS_XZ, 60.0, 150.0, -180.0, -110.0, 548.7, True, m["light"], (30.0, 24.0, 18.0))
    be.rect(scenes.AXIS_XZ, 380.0, 480.0, -460.0, -380.0, 548.7, True, m["light"], (8.0, 12.0, 20.0))


def _panels(be, m):
    be.rect(scenes.AXIS_XZ, 90.0, 260.0, -330.0, -160.0, 210.0, False, m["white"], None)        # a two-sided panel above the floor
    be.rect(scenes.AXIS_XY, 300.0, 480.0, 20.0, 300.0, -200.0, True, m["white"], None)          # and an upright one


SCENES = {   # name: (builder of the scene at W x W, the shadow kernel the selector must pick, primitives, shadow planes)
    "cornell": (lambda W: scenes.build_cornell(scenes.HostBackend("cornell"), W, W, lambert_only=False), "pair", 32, 2),
    "floor_lamp": (lambda W: scenes.build_lamp_box(scenes.HostBackend("floor_lamp"), W, W, _floor_lamp, full_materials=True), "pair", 32, 2),
    "three_lights": (lambda W: _small_box("three_lights", W, _three_lamps), "pair", 23, 3),
    "rect_lights": (lambda W: _small_box("rect_lights", W, _two_rect_lamps, _panels), "pair", 24, 2),
    "one_light": (lambda W: scenes.build_lamp_box(scenes.HostBackend("one_light"), W, W, scenes.lamp_rect(), full_materials=True), "flat", 31, 1),
    "34_prims": (lambda W: scenes.build_cornell(scenes.HostBackend("cornell34"), W, W, lambert_only=False, extras=_panels), "flat", 34, 2),
}


def _reserved(generic):
    return (C.c_int32 * 8)(1 if generic else 0)


def _render(ctx, params, generic, lanes, **opt):
    """lanes 0: the default lane count"""
    ctx.set_options(lanes=lanes, reserved=_reserved(generic), **opt)
    try:
        film = ctx.render(params)
        c = ctx.counters()
    finally:
        ctx.set_options()
    return film, (c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded)


def _both_ways(ctx, name, W, spp, depth, **opt):
    """the scene's film with the generic kernels and with the ones the selector picks, at one lane and at the default lane count: the same bits and the same
    four counters; returns (scene, film, counters)"""
    be = SCENES[name][0](W)
    ctx.upload(be.flatten())
    params = jp.render_params(W, W, spp, depth, 1234)
    film0, cnt0 = _render(ctx, params, True, 1, **opt)
    assert np.isfinite(film0).all()
    for generic, lanes in ((False, 1), (True, 0), (False, 0)):
        film, cnt = _render(ctx, params, generic, lanes, **opt)
        assert np.array_equal(film.view(np.uint32), film0.view(np.uint32)), "generic=%d lanes=%d: %d pixels differ" % (generic, lanes, (film != film0).any(-1).sum())
        assert cnt == cnt0, (generic, lanes, cnt, cnt0)
    return be, params, film0, cnt0


# ---- which kernel runs -----------------------------------------------------------------------------------------------------------------
def test_selector_choice(ctx):
    """the pair kernel where k_shadow<2, FeatFlat> was chosen AND the scene has <= 32 primitives AND two or more shadow planes; reserved[0] = 1 keeps the
    generic kernel everywhere"""
    for name, (build, want, n_prims, n_planes) in SCENES.items():
        be = build(32)
        info = jp.describe_upload(be.flatten())
        assert (info.trav_mode, info.n_prims, info.n_planes) == (2, n_prims, n_planes), (name, info.trav_mode, info.n_prims, info.n_planes)
        ctx.upload(be.flatten())
        assert ctx.shadow_kernel() == want, (name, ctx.shadow_kernel())
        ctx.set_options(reserved=_reserved(True))
        try:
            assert ctx.shadow_kernel() == "generic", name
        finally:
            ctx.set_options()
        assert ctx.shadow_kernel() == want, name


# ---- the Cornell box: frame sizes, sample counts, depths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,spp", [(8, 1), (8, 4), (16, 1), (24, 3), (32, 7), (64, 16)])
def test_cornell_frames(ctx, W, spp):
    _, _, film, cnt = _both_ways(ctx, "cornell", W, spp, 5)
    assert film.mean() > 0.02 and cnt[2] > W * W * spp and 0 < cnt[3] < cnt[2]          # more shadow rays than paths: two-ray entries; some occluded


def test_cornell_against_the_oracle(H, ctx):
    be, params, film, cnt = _both_ways(ctx, "cornell", 32, 8, 5)
    ref, rc = H.oracle_render(be.flatten(), params, 4)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()
    assert cnt == (rc.closest_rays, rc.closest_hits, rc.shadow_rays, rc.shadow_occluded)


@pytest.mark.parametrize("depth", [1, 0])
def test_cornell_shallow(ctx, depth):
    """maxDepth 1: one shadow launch per batch; maxDepth 0: none that does work"""
    _, _, film, cnt = _both_ways(ctx, "cornell", 32, 4, depth)
    assert (cnt[2] > 0) == (depth > 0)


def test_regions_beyond_one_block(ctx):
    """512-slot regions (131072 paths over 256 workgroups... one per CU): threads take a second entry of their region, with the prefetched directions"""
    _, _, film, cnt = _both_ways(ctx, "cornell", 128, 8, 2, blocks_per_cu=1)
    assert cnt[2] > 128 * 128 * 8


# ---- the other entry shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,spp", [(16, 2), (64, 5)])
@pytest.mark.parametrize("name", ["floor_lamp", "three_lights", "rect_lights", "one_light", "34_prims"])
def test_other_scenes(ctx, name, W, spp):
    _, _, film, cnt = _both_ways(ctx, name, W, spp, 5)
    assert film.mean() > 0.005 and cnt[2] > 0
    if name == "three_lights":
        assert cnt[2] > 2 * W * W * spp, cnt                                             # three rays at most of the first hits: odd last rays abound


def test_rectangles_against_the_oracle(H, ctx):
    be, params, film, cnt = _both_ways(ctx, "rect_lights", 32, 8, 5)
    ref, rc = H.oracle_render(be.flatten(), params, 4)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()
    assert cnt == (rc.closest_rays, rc.closest_hits, rc.shadow_rays, rc.shadow_occluded)
