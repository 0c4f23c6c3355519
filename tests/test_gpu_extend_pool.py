"""k_extend_pool / k_trace_pool (csrc/jp_kernels.hip, flat_prims_pool in csrc/jp_device.h; DESIGN.md section 5, "Pooled closest hits"): the closest-hit
kernel of the flat-shape scenes with <= 32 primitives tests a wave's candidates from one pooled list.  Every hit record must be the sequential loop's, so
every scene here is rendered with the generic kernels (JpOptions.reserved[0] = 1) and with the ones the selector picks, at one lane and at the default lane
count: the films must be the same bits and the four ray counters equal; the Cornell box and a scene of rectangles are held to the oracle's bits too.
Through jp_trace (k_trace_pool against k_trace<2>) the hit records themselves are compared, bit for bit, on ray groups chosen for what the pooled pass
does differently: waves of one octant (long candidate lists in every lane), mixed waves, waves whose even lanes carry no candidate at all, axis-parallel
rays, origins on the walls, rays that all leave the camera position, finite far ends, a negative tmin (the wave then takes the sequential loop), a batch
whose last wave is partial, and a scene with a duplicated box whose every hit is an exact distance tie of two primitives.

Region fills: 8 x 8 at 1 spp is one region of at most 64 rays (one wave, partly filled at the later bounces), from there up to 64 x 64 at 16 spp; a small
max_slots gives many short batches whose regions are partly filled from the first bounce on."""
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


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _small_box(name, W, lamp, extras=None):
    """the Cornell box without its short box (20 primitives) and without a light: lamp(be, mats) and extras(be, mats) add the rest"""
    be = scenes.HostBackend(name)
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    front = lookat - lookfrom
    be.camera(lookfrom, (front / np.linalg.norm(front)).astype(np.float32), (0, 1, 0), 60.0, W, W)
    red = be.mat_matte((0.63, 0.065, 0.05)); green = be.mat_matte((0.14, 0.45, 0.091)); white = be.mat_matte((0.725, 0.71, 0.68))
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    m = dict(white=white, red=red, light=be.mat_matte((0.65, 0.65, 0.65)))
    A = scenes.cornell_assets(); T = scenes.cornell_textured_assets()
    lamp(be, m)
    for path, mat in ((T["floor_only"], white), (T["ceiling"], white), (T["back"], white), (A["tallbox"], golden), (A["left"], red), (A["right"], green)):
        be.mesh(path, True, True, mat=mat)
    if extras:
        extras(be, m)
    be.preprocess()
    return be


def _two_rect_lamps(be, m):
    be.rect(scenes.AXIS_XZ, 60.0, 150.0, -180.0, -110.0, 548.7, True, m["light"], (30.0, 24.0, 18.0))
    be.rect(scenes.AXIS_XZ, 380.0, 480.0, -460.0, -380.0, 548.7, True, m["light"], (8.0, 12.0, 20.0))


def _panels(be, m):
    be.rect(scenes.AXIS_XZ, 90.0, 260.0, -330.0, -160.0, 210.0, False, m["white"], None)        # a two-sided panel above the floor
    be.rect(scenes.AXIS_XY, 300.0, 480.0, 20.0, 300.0, -200.0, True, m["white"], None)          # and an upright one


def _second_tall_box(be, m):
    be.mesh(scenes.cornell_assets()["tallbox"], True, True, mat=m["red"])                       # the tall box once more, in red: ten exact duplicates


SCENES = {   # name: (builder of the scene at W x W, the closest-hit kernel the selector must pick, primitives)
    "cornell": (lambda W: scenes.build_cornell(scenes.HostBackend("cornell"), W, W, lambert_only=False), "pool", 32),            # exactly 32: the last scene of the 32-bit mask
    "rects": (lambda W: _small_box("rects", W, _two_rect_lamps, _panels), "pool", 24),
    "twin_box": (lambda W: _small_box("twin_box", W, scenes.lamp_mesh(1, 1), _second_tall_box), "pool", 32),
    "34_prims": (lambda W: scenes.build_cornell(scenes.HostBackend("cornell34"), W, W, lambert_only=False, extras=_panels), "flat", 34),
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
    four counters; returns (scene, params, film, counters)"""
    be = SCENES[name][0](W)
    ctx.upload(be.flatten())
    assert ctx.extend_kernel() == SCENES[name][1]
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
    """the pooled kernel where k_extend<2, FeatFlat> was chosen AND the scene has <= 32 primitives: exactly 32 takes it, 34 keeps today's kernel;
    reserved[0] = 1 keeps the generic kernel everywhere"""
    for name, (build, want, n_prims) in SCENES.items():
        be = build(32)
        info = jp.describe_upload(be.flatten())
        assert (info.trav_mode, info.n_prims) == (2, n_prims), (name, info.trav_mode, info.n_prims)
        ctx.upload(be.flatten())
        assert ctx.extend_kernel() == want, (name, ctx.extend_kernel())
        ctx.set_options(reserved=_reserved(True))
        try:
            assert ctx.extend_kernel() == "generic", name
        finally:
            ctx.set_options()
        assert ctx.extend_kernel() == want, name


# ---- films and counters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,spp", [(8, 1), (8, 4), (16, 1), (24, 3), (32, 7), (64, 16)])
def test_cornell_frames(ctx, W, spp):
    _, _, film, cnt = _both_ways(ctx, "cornell", W, spp, 5)
    assert film.mean() > 0.02 and cnt[0] > W * W * spp and 0 < cnt[1] <= cnt[0]


@pytest.mark.parametrize("depth", [1, 0])
def test_cornell_shallow(ctx, depth):
    """maxDepth 1: camera rays and one bounce; maxDepth 0: camera rays only"""
    _, _, film, cnt = _both_ways(ctx, "cornell", 32, 4, depth)
    assert cnt[0] >= 32 * 32 * 4 and cnt[1] > 0


def test_short_batches(ctx):
    """max_slots = one sample per pixel a batch of a 24 x 24 frame: 576 paths over the workgroups, regions of a few rays, nearly every wave partly filled"""
    _, _, film, cnt = _both_ways(ctx, "cornell", 24, 5, 5, max_slots=24 * 24)
    assert cnt[0] > 24 * 24 * 5


def test_regions_beyond_one_block(ctx):
    """512-slot regions (one workgroup per CU): a wave takes a second pass through its region, with the prefetched ray"""
    _, _, film, cnt = _both_ways(ctx, "cornell", 128, 8, 2, blocks_per_cu=1)
    assert cnt[0] > 128 * 128 * 8


@pytest.mark.parametrize("name", ["rects", "twin_box", "34_prims"])
def test_other_scenes(ctx, name):
    _, _, film, cnt = _both_ways(ctx, name, 48, 5, 5)
    assert film.mean() > 0.005 and cnt[1] > 0


@pytest.mark.parametrize("name", ["cornell", "rects"])
def test_against_the_oracle(H, ctx, name):
    be, params, film, cnt = _both_ways(ctx, name, 32, 8, 5)
    ref, rc = H.oracle_render(be.flatten(), params, 4)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "%d pixels differ from the oracle" % (film != ref).any(-1).sum()
    assert cnt == (rc.closest_rays, rc.closest_hits, rc.shadow_rays, rc.shadow_occluded)


# ---- hit records through jp_trace --------------------------------------------------------------------------------------------------------
CAMERA = np.array([278.0, 273.0, 960.0], np.float32)


def _trace_rays():
    """4096 + 37 rays in groups of 64 (a wave of k_trace_pool takes 64 consecutive rays; the last wave holds 37)"""
    rng = np.random.default_rng(23)
    n = 4096 + 37
    g = np.arange(n) // 64
    o = np.stack([rng.uniform(5.0, 550.0, n), rng.uniform(5.0, 540.0, n), rng.uniform(-555.0, -5.0, n)], -1).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tmin = np.full(n, 0.001, np.float32); tmax = np.full(n, np.inf, np.float32)
    octant = np.array([[1 if (k >> a) & 1 else -1 for a in range(3)] for k in range(8)], np.float32)
    one = g < 16                                                         # groups 0-15: one octant each; 16-23: mixed
    d[one] = np.abs(d[one]) * octant[g[one] % 8]
    odd = (g >= 24) & (g < 32)                                           # 24-31: only the odd lanes live -- the even ones start outside the box and point away from it
    dead = odd & (np.arange(n) % 2 == 0)
    o[dead] = np.array([278.0, 2000.0, -280.0], np.float32); d[dead] = np.array([0.0, 1.0, 0.0], np.float32)
    ax = (g >= 32) & (g < 40)                                            # 32-39: axis-parallel rays, zeros of both signs in the other components
    k = rng.integers(0, 3, n); sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    par = np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0); par[np.arange(n), k] = sgn
    d[ax] = par[ax].astype(np.float32)
    wall = (g >= 40) & (g < 48)                                          # 40-47: origins exactly on the planes of the walls, floor, ceiling and back
    planes = [np.array([0.0, 549.6, 556.0], np.float32), np.array([0.0, 548.8], np.float32), np.array([0.0, -559.2], np.float32)]
    for i in np.nonzero(wall)[0]:
        a = int(rng.integers(0, 3)); o[i, a] = rng.choice(planes[a])
    cam = (g >= 48) & (g < 56)                                           # 48-55: every ray from the camera position, into the box
    tgt = np.stack([rng.uniform(0.0, 556.0, n), rng.uniform(0.0, 548.0, n), rng.uniform(-559.0, 0.0, n)], -1)
    dc = tgt - CAMERA[None, :]; dc = (dc / np.linalg.norm(dc, axis=1, keepdims=True)).astype(np.float32)
    o[cam] = CAMERA; d[cam] = dc[cam]
    far = (g >= 56) & (g < 60)                                           # 56-59: finite far ends, some below tmin
    tmax[far] = rng.uniform(50.0, 600.0, n).astype(np.float32)[far]
    tmax[far & (np.arange(n) % 7 == 0)] = np.float32(0.0005)
    tmin[(g >= 60) & (g < 62)] = rng.uniform(0.0, 300.0, n).astype(np.float32)[(g >= 60) & (g < 62)]   # 60-61: the caller's own tmin, zero and large
    tmin[(g == 62) & (np.arange(n) % 5 == 0)] = np.float32(-10.0)        # 62: a negative tmin in some lanes; 63 and the partial wave 64: plain
    return o, d, tmin, tmax


def _trace_both(ctx, name, o, d, tmin, tmax):
    be = SCENES[name][0](64)
    ctx.upload(be.flatten())
    out = []
    for generic in (True, False):
        ctx.set_options(reserved=_reserved(generic))
        try:
            out.append(ctx.trace(o, d, tmin, tmax))
        finally:
            ctx.set_options()
    (h0, t0, p0, n0), (h1, t1, p1, n1) = out
    bad = (h0 != h1) | (p0 != p1) | (t0.view(np.uint32) != t1.view(np.uint32)) | (n0.view(np.uint32) != n1.view(np.uint32)).any(-1)
    assert not bad.any(), "%d hit records differ, first ray %d: generic (%d, %r, %d) pooled (%d, %r, %d)" % (bad.sum(), np.argmax(bad), h0[np.argmax(bad)], t0[np.argmax(bad)], p0[np.argmax(bad)],
                                                                                                          h1[np.argmax(bad)], t1[np.argmax(bad)], p1[np.argmax(bad)])
    return h0, t0, p0


@pytest.mark.parametrize("name", ["cornell", "rects"])
def test_trace_hit_records(ctx, name):
    o, d, tmin, tmax = _trace_rays()
    h, t, p = _trace_both(ctx, name, o, d, tmin, tmax)
    g = np.arange(len(o)) // 64
    assert h.sum() > len(o) // 2 and (h == 0).sum() > 16
    assert h[(g >= 24) & (g < 32)].reshape(-1, 2)[:, 0].sum() == 0 and h[(g >= 24) & (g < 32)].reshape(-1, 2)[:, 1].sum() > 200   # the even lanes hit nothing, the odd ones do
    assert h[g == 64].sum() > 10                                          # the partial wave's rays were traced


def test_trace_exact_ties(ctx):
    """twin_box: the tall box twice, so every hit on it is an exact distance tie between a primitive and its duplicate.  Rays from the camera position and from
    inside the room at the box: the records must be the sequential loop's (the first of the two in the mask's order; which copy that is depends on the tree)"""
    rng = np.random.default_rng(29)
    n = 3000
    o = np.where((np.arange(n) < n // 2)[:, None], CAMERA[None, :], np.stack([rng.uniform(5.0, 550.0, n), rng.uniform(5.0, 540.0, n), rng.uniform(-555.0, -5.0, n)], -1)).astype(np.float32)
    tgt = np.stack([rng.uniform(265.0, 472.0, n), rng.uniform(0.0, 330.0, n), rng.uniform(-456.0, -247.0, n)], -1)       # the tall box's extent
    d = tgt - o; d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    h, t, p = _trace_both(ctx, "twin_box", o, d, np.full(n, 0.001, np.float32), np.full(n, np.inf, np.float32))
    on_box = (h > 0) & (((p >= 8) & (p < 18)) | (p >= 22))                # the caller's ids: lamp 0-1, floor / ceiling / back 2-7, the box 8-17, walls 18-21, its twin 22-31
    assert on_box.sum() > n // 3, on_box.sum()
