"""The thin-lens camera on the MI355X (INTEGRATION.md "Lens"): the hook against the host function bit for bit, no lens is a no-op, the film of an emitter
against jp_trace over the hooked rays exactly, the circle of confusion, guides and the other integrators, the schedules, the certified walk, autofocus,
the host API and the command line, device memory.  Films are at most 48 x 32 at <= 64 spp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import lens_ref as R
import normals_ref as NR

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARGUMENT = -1
W, Hh = 32, 24
EYE = np.array([10.0, -4.0, 30.0])                                # the emitter scenes' camera: looks along -z, up +y; |up| = tan(fov / 2) = 1: the film spans +-F / 2 vertically on the plane of focus
VFOV = 90.0


@pytest.fixture()
def ctx():
    """a context of its own per test: the lens is context state"""
    c = jp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell():
    be = scenes.build_cornell(scenes.HostBackend("lens_cornell"), W, Hh, lambert_only=False)
    return be, be.flatten()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _pixels(w, h, spp):
    """x, y, s of every sample of every pixel, pixel-major (row-major pixels, samples in order)"""
    yy, xx, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xx.ravel().astype(np.int32), yy.ravel().astype(np.int32), ss.ravel().astype(np.int32)


def _resolve(v, spp):
    """k_resolve's expression for per-sample values v (npix, spp, k): L = 0; L = L + v_s * (1.0f / spp) in sample order; 0.f + Clamp01(L)"""
    ratio = f32(1.0) / f32(spp)
    L = np.zeros(v.shape[::2], f32)
    for s in range(spp):
        L = (L + (v[:, s].astype(f32) * ratio).astype(f32)).astype(f32)
    return (f32(0.0) + np.clip(L, f32(0.0), f32(1.0))).astype(f32)


def _trace_all(ctx, o, d):
    n = len(o)
    return ctx.trace(o, d, np.full(n, 1e-3, f32), np.full(n, np.inf, f32))


def _emitter(z, rho, extra=None):
    """one emissive disk of radius rho facing the camera at depth z on its axis, radiance (1, 1, 1), a black material; nothing else, no background"""
    be = scenes.HostBackend("lens_emitter")
    be.camera(tuple(EYE), (0, 0, -1), (0, 1, 0), VFOV, W, Hh)
    be.disk((EYE[0], EYE[1], EYE[2] - z), (0, 0, 1), rho, be.mat_matte((0.0, 0.0, 0.0)), (1.0, 1.0, 1.0))
    if extra:
        extra(be)
    be.preprocess()
    return be


def _focus_plane_boxes(cam, F):
    """per pixel the extent of its footprint on the plane of focus in lens-axis coordinates: (x0, x1, y0, y1), each (Hh, W)"""
    lr = np.linalg.norm(list(cam.right)); lu = np.linalg.norm(list(cam.up))
    x = np.arange(W + 1) / W - 0.5; y = 0.5 - np.arange(Hh + 1) / Hh
    X = F * lr * x; Y = F * lu * y
    x0, y1 = np.meshgrid(X[:-1], Y[:-1]); x1, y0 = np.meshgrid(X[1:], Y[1:])
    return x0, x1, y0, y1


def _grown(box, m):
    x0, x1, y0, y1 = box
    return x0 - m, x1 + m, y0 - m, y1 + m


def _corners(box):
    x0, x1, y0, y1 = box
    return [(x0, y0), (x0, y1), (x1, y0), (x1, y1)]


# ---- G1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blades,rot", [(0, 0.0), (3, 0.0), (6, 11.0), (16, -27.5)])
def test_hook_is_the_host_function(ctx, cornell, blades, rot):
    be, sp = cornell
    ctx.upload(sp)
    cam = sp.contents.camera
    rng = np.random.default_rng(9)
    n = 5000
    x = rng.integers(0, W, n).astype(np.int32); y = rng.integers(0, Hh, n).astype(np.int32); s = rng.integers(0, 4096, n).astype(np.int32)
    p = jp.render_params(W, Hh, 1, 5, 4242)
    o0, d0, k0 = ctx.camera_rays(p, x, y, s)                       # no lens: the pinhole, the first bounce draws from dim 2
    fxfy, u = R.sample_draws(4242, x, y, s)
    ho, hd = jp.lens_rays(cam, None, fxfy)
    assert (k0 == 2).all() and _same(o0, ho) and _same(d0, hd)
    lens = jp.lens(20.0, 700.0, blades, rot)
    ctx.set_lens(lens)
    o, d, k = ctx.camera_rays(p, x, y, s)
    ho, hd = jp.lens_rays(cam, lens, fxfy, u)
    assert (k == 4).all()
    exact = blades != 0 or ctx.build_info().libm_sincosf != 0
    if exact:
        assert _same(o, ho) and _same(d, hd)
    else:                                                          # a host libm the device does not reproduce: the disk's sine / cosine may differ in the last place
        assert np.abs(o - ho).max() <= 2e-4 and np.abs(d - hd).max() <= 1e-6
    assert np.abs(o - np.array(list(cam.pos), f32)).max() > 5.0    # the origins are on the aperture, not at the eye
    # JP_SAMPLER_DEBUG: (0.5, 0.5) is the centre of the disk (and of a polygon with an even number of blades)
    pd = jp.render_params(W, Hh, 1, 5, 4242, sampler_mode=jp.JP_SAMPLER_DEBUG)
    od, dd, kd = ctx.camera_rays(pd, x, y, s)
    fd, ud = R.sample_draws(4242, x, y, s, debug=True)
    hod, hdd = jp.lens_rays(cam, lens, fd, ud)
    assert (kd == 4).all() and _same(od, hod) and _same(dd, hdd)
    if blades % 2 == 0:
        assert (od == np.array(list(cam.pos), f32)[None]).all()
    info = ctx.lens_info()
    assert (info.radius, info.focus_distance, info.blades, info.rotation_deg) == (20.0, 700.0, blades, f32(rot))


# ---- G2 -------------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(ctx, cornell):
    be, sp = cornell
    ctx.upload(sp)
    p = jp.render_params(W, Hh, 8, 5, 1234)

    def shot():
        film = ctx.render(p); c = ctx.counters()
        assert ctx.lens_info().lens_last_render == 0
        return film, (c.samples, c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded), ctx.render_guides(p, 2)
    base = shot()
    ctx.set_lens(None); null = shot()
    ctx.set_lens(0.0, 0.0); zero = shot()
    ctx.set_lens(15.0, 700.0); film_on = ctx.render(p)
    assert ctx.lens_info().lens_last_render == 1 and not _same(film_on, base[0])
    ctx.set_lens(None); back = shot()
    for other in (null, zero, back):
        assert _same(other[0], base[0]) and other[1] == base[1]
        assert all(_same(a, b) for a, b in zip(other[2], base[2]))
    assert base[0].mean() > 0.05


# ---- G3 -------------------------------------------------------------------------------------------------------------------------------------------
def _film_from_hooked_rays(ctx, p):
    x, y, s = _pixels(p.width, p.height, p.spp)
    o, d, _ = ctx.camera_rays(p, x, y, s)
    hit = _trace_all(ctx, o, d)[0]
    v = np.repeat(hit.reshape(-1, p.spp, 1).astype(f32), 3, -1)
    return _resolve(v, p.spp).reshape(p.height, p.width, 3)


@pytest.mark.parametrize("blades", [0, 3])
@pytest.mark.parametrize("z", [4.0, 9.0])                          # in front of and behind the plane of focus (F = 6)
def test_film_is_made_of_the_hooked_rays(ctx, blades, z):
    be = _emitter(z, 0.8)
    ctx.upload(be.flatten())
    p = jp.render_params(W, Hh, 16, 0, 99)                         # max_depth 0: a path is its first hit's emission, 1 or 0
    pin = ctx.render(p)
    assert _same(pin, _film_from_hooked_rays(ctx, p)) and 0.0 < pin.mean() < 0.5 and set(np.unique(pin * 16)) <= set(range(17))
    ctx.set_lens(1.5, 6.0, blades, 10.0)
    film = ctx.render(p)
    assert ctx.lens_info().lens_last_render == 1
    assert _same(film, _film_from_hooked_rays(ctx, p))
    assert not _same(film, pin) and ((film > 0) & (film < 1)).sum() > ((pin > 0) & (pin < 1)).sum()      # blurred: more partly covered pixels


# ---- G4 -------------------------------------------------------------------------------------------------------------------------------------------
F4, R4, RT = 6.0, 3.0, 6.0                                         # focus distance; lens radius of the disk cases and of the triangle cases


def _coc_films(ctx, z, rho, blades, radius, spp=64, seeds=8):
    be = _emitter(z, rho)
    ctx.upload(be.flatten())
    ctx.set_lens(radius, F4, blades, 0.0)
    films = [ctx.render(jp.render_params(W, Hh, spp, 0, 500 + 31 * k)) for k in range(seeds)]
    return be.flatten().contents.camera, np.array([f[..., 0] for f in films], np.float64)


def _z_of(films, mask, expected):
    assert mask.sum() >= 12
    means = films[:, mask].mean(-1)
    se = means.std(ddof=1) / np.sqrt(len(means))                   # the bound of test_gpu_mis.py: the films' means against the closed form, |z| <= 5
    z = (means.mean() - expected) / se
    print("%d plateau pixels: mean %.5f vs %.5f expected, z = %.2f" % (mask.sum(), means.mean(), expected, z))
    return z


def _box_distances(box):
    """nearest and farthest distance from the axis to each pixel's box"""
    x0, x1, y0, y1 = box
    dx = np.maximum(np.maximum(x0, -x1), 0.0); dy = np.maximum(np.maximum(y0, -y1), 0.0)
    far = np.max([np.hypot(a, b) for a, b in _corners(box)], 0)
    return np.hypot(dx, dy), far


@pytest.mark.parametrize("z", [4.0, 9.0])
def test_circle_of_confusion_disk(ctx, z):
    rho = 0.2
    k = abs(1.0 - z / F4)
    assert rho < R4 * k
    cam, films = _coc_films(ctx, z, rho, 0, R4)
    px = F4 * np.linalg.norm(list(cam.up)) / Hh                    # one pixel on the plane of focus
    box = _focus_plane_boxes(cam, F4)
    near, _ = _box_distances(_grown(box, px))                      # one pixel of margin
    outside = near > (rho + R4 * k) * F4 / z
    assert outside.sum() > 300 and not films[:, outside].any()      # exactly 0
    _, far = _box_distances(box)
    plateau = far < (R4 * k - rho) * F4 / z
    zs = _z_of(films, plateau, rho ** 2 / (R4 * (1.0 - z / F4)) ** 2)
    assert abs(zs) <= 5.0
    assert films.max() < 0.99


def _lens_centre(qx, qy, z):
    """the centre, in units of the lens radius, of the disk of lens points whose rays through focus-plane point q reach the emitter"""
    c = F4 / z - 1.0
    return -qx / c / RT, -qy / c / RT


RHO0 = 0.6                                                         # radius of that disk of lens points when the emitter's radius is RHO0 * |1 - z / F|


@pytest.mark.parametrize("z", [4.0, 12.0])                         # F / z - 1 = +0.5 and -0.5: mirror images when rho follows |1 - z / F|
def test_circle_of_confusion_triangle(ctx, z):
    cam, films = _coc_films(ctx, z, RHO0 * abs(1.0 - z / F4), 3, RT)
    px = F4 * np.linalg.norm(list(cam.up)) / Hh
    box = _focus_plane_boxes(cam, F4)
    corners = [_lens_centre(a, b, z) for a, b in _corners(_grown(box, px))]
    rad = np.array([np.hypot(a, b) for a, b in corners])
    # exactly zero wherever the disk of lens points misses the triangle: the pixel's grown footprint lies beyond one edge line by more than the disk's radius --
    # which includes pixels between the triangle and its circumcircle
    v = R.vertices(3, 0.0); e = v[1:] - v[:-1]
    nrm = np.stack([-e[:, 1], e[:, 0]], -1); nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    per_edge = np.array([[(a - v[j, 0]) * nrm[j, 0] + (b - v[j, 1]) * nrm[j, 1] for a, b in corners] for j in range(3)])     # (edge, corner, Hh, W)
    beyond = (per_edge.max(1) < -(RHO0 / RT)).any(0)
    ring = beyond & (rad.max(0) < 1.0)
    print("%d pixels beyond an edge, %d of them inside the circumcircle" % (beyond.sum(), ring.sum()))
    assert ring.sum() >= 6 and beyond.sum() > 200 and not films[:, beyond].any()
    inner = [_lens_centre(a, b, z) for a, b in _corners(box)]
    sd = np.array([R.inside_polygon(a.ravel(), b.ravel(), 3, 0.0).reshape(Hh, W) for a, b in inner])     # signed distance to the nearest edge, lens radii
    plateau = sd.min(0) > RHO0 / RT
    zs = _z_of(films, plateau, np.pi * RHO0 ** 2 / (RT ** 2 * R.polygon_area(3)))
    assert abs(zs) <= 5.0
    # the sign: vertex 0 of the triangle lies along +right.  The lens centre of q is -q / (F / z - 1): for z < F the vertex's image points to -right and the film is
    # empty beyond the opposite edge's image on the +right side; for z > F the other way round
    c = abs(F4 / z - 1.0)
    reach = c * (0.5 * RT + RHO0) + px                             # the opposite edge's image, the disk and a pixel of margin
    x0, x1, _, _ = box
    lit = films.sum(0)
    left = lit[x1 < -reach].sum(); right = lit[x0 > reach].sum()
    print("z = %g: film mass beyond %.2f on the left %.3f, on the right %.3f" % (z, reach, left, right))
    assert (left > 0.2 and right == 0.0) if z < F4 else (right > 0.2 and left == 0.0)


def test_triangle_images_are_point_mirrors(ctx):
    near = _coc_films(ctx, 4.0, RHO0 * abs(1.0 - 4.0 / F4), 3, RT)[1].mean(0)
    far = _coc_films(ctx, 12.0, RHO0 * abs(1.0 - 12.0 / F4), 3, RT)[1].mean(0)
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    mirrored, plain = corr(near, far[::-1, ::-1]), corr(near, far)  # the film is symmetric about its centre: the point mirror is the double flip
    print("correlation of the z < F film with the z > F film: %.3f point-mirrored, %.3f as it is" % (mirrored, plain))
    assert mirrored > 0.8 and mirrored > plain + 0.15
    assert abs(near.sum() - far.sum()) <= 0.1 * near.sum()


# ---- G5 -------------------------------------------------------------------------------------------------------------------------------------------
def test_guides_and_the_other_integrators(ctx, cornell):
    be, sp = cornell
    ctx.upload(sp)
    ctx.set_lens(25.0, 650.0, 5, 12.0)
    spp = 4
    p = jp.render_params(W, Hh, spp, 5, 808)
    x, y, s = _pixels(W, Hh, spp)
    o, d, _ = ctx.camera_rays(p, x, y, s)
    hit, t, prim, nrm = _trace_all(ctx, o, d)
    assert 0 < hit.sum() and len(np.unique(prim)) > 5
    tt = np.where(hit > 0, t, f32(0)).astype(f32).reshape(-1, spp, 1)
    nn = np.where(hit[:, None] > 0, nrm, f32(0)).astype(f32).reshape(-1, spp, 3)
    inv = f32(1.0) / f32(spp)

    def mean(v):                                                   # acc = 0; acc += v_s in sample order; acc * (1.0f / spp)
        acc = np.zeros((v.shape[0], v.shape[2]), f32)
        for k in range(spp):
            acc = (acc + v[:, k]).astype(f32)
        return (acc * inv).astype(f32)
    alb, gn, gz = ctx.render_guides(p, spp)
    assert _same(gz.reshape(-1, 1), mean(tt)) and _same(gn.reshape(-1, 3), mean(nn))
    pin = jp.Context(0)
    try:
        pin.upload(sp)
        assert not _same(pin.render_guides(p, spp)[2], gz)
    finally:
        pin.close()
    # the debug-normal integrator: the same rays, the normal as a colour, k_resolve's sum
    pn = jp.render_params(W, Hh, spp, 5, 808, integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL)
    film = ctx.render(pn)
    assert ctx.lens_info().lens_last_render == 1
    assert _same(film.reshape(-1, 3), _resolve(nn, spp))
    # Whitted renders with a lens
    pw = jp.render_params(W, Hh, spp, 5, 808, integrator=jp.JP_INTEGRATOR_WHITTED)
    fw = ctx.render(pw)
    assert np.isfinite(fw).all() and fw.mean() > 0.05 and ctx.lens_info().lens_last_render == 1
    ctx.set_lens(None)
    assert not _same(ctx.render(pw), fw)


# ---- G6 -------------------------------------------------------------------------------------------------------------------------------------------
def test_schedules(ctx):
    w, h = 48, 32
    be = scenes.build_cornell(scenes.HostBackend("lens_cornell_48"), w, h, lambert_only=False)
    ctx.upload(be.flatten())
    ctx.set_lens(18.0, 700.0, 6, 5.0)
    full = ctx.render(jp.render_params(w, h, 8, 5, 77))
    shards = [ctx.render(jp.render_params(w, h, 8, 5, 77, band_rows=4, shard_index=k, shard_count=3)) for k in range(3)]
    assert all(sh.any() for sh in shards) and _same(shards[0] + shards[1] + shards[2], full)
    ctx.set_options(lanes=1); one = ctx.render(jp.render_params(w, h, 8, 5, 77))
    assert ctx.build_info().lanes_last_render == 1
    ctx.set_options(); ctx.set_options(lanes=3); three = ctx.render(jp.render_params(w, h, 8, 5, 77))
    assert ctx.build_info().lanes_last_render == 3
    ctx.set_options()
    assert _same(one, full) and _same(three, full)
    rgb8, film = ctx.render_rgb8(jp.render_params(w, h, 8, 5, 77), with_film=True)
    enc = np.zeros(film.size, np.uint8)
    jp.host_lib().jp_host_gamma_encode(film.ctypes.data_as(C.c_void_p), film.size, enc.ctypes.data_as(C.c_void_p))
    assert _same(film, full) and np.array_equal(rgb8.reshape(-1), enc)
    # the fused schedule falls back with a lens, and runs again without
    ctx.set_options(fused=1)
    fused = ctx.render(jp.render_params(w, h, 8, 5, 77))
    assert ctx.build_info().fused_last_render == 0 and _same(fused, full)
    ctx.set_lens(None); ctx.render(jp.render_params(w, h, 8, 5, 77))
    assert ctx.build_info().fused_last_render == 1
    ctx.set_options()
    # refusals leave the lens in force and the context usable
    ctx.set_lens(18.0, 700.0, 6, 5.0)
    for bad, word in ((jp.lens(-1.0, 700.0), "radius"), (jp.lens(18.0, 0.0), "focus_distance"), (jp.lens(18.0, 700.0, 2), "blades"), (jp.lens(18.0, 700.0, 6, float("nan")), "rotation_deg")):
        assert ctx.lib.jp_set_lens(ctx.h, C.byref(bad)) == INVALID_ARGUMENT and word in ctx.lib.jp_last_error().decode()
    assert ctx.lens_info().blades == 6
    assert _same(ctx.render(jp.render_params(w, h, 8, 5, 77)), full)
    x = np.array([0, w], np.int32); y = np.array([0, 0], np.int32); s = np.zeros(2, np.int32)
    with pytest.raises(jp.JetPbrtError, match="out of range"):
        ctx.camera_rays(jp.render_params(w, h, 1), x, y, s)
    empty = jp.Context(0)
    try:
        with pytest.raises(jp.JetPbrtError, match="no scene"):
            empty.camera_rays(jp.render_params(w, h, 1), x[:1], y[:1], s[:1])
        with pytest.raises(jp.JetPbrtError, match="no scene"):
            empty.focus_distance(1.0, 1.0)
    finally:
        empty.close()


# ---- G7 -------------------------------------------------------------------------------------------------------------------------------------------
def _ico_scene(certified):
    p = os.path.join(scenes.asset_dir(), "lens_icosphere_3.obj")
    v, f = NR.icosphere(3, 1.0, NR.generic_rotation())
    be = scenes.HostBackend("lens_ico")
    be.set_reference_tree(True, certified=certified)
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), 40.0, 24, 16)
    be.envlight((0.4, 0.5, 0.7))
    be.pointlight((3.0, -3.0, 4.0), (30.0, 30.0, 30.0))
    be.mesh(scenes.write_obj(p, v.astype(f32), f), False, False, mat=be.mat_matte((0.6, 0.6, 0.6)))
    be.preprocess()
    return be


def test_certified_walk_with_a_lens(ctx):
    films = {}
    for certified in (False, True):
        be = _ico_scene(certified)
        sp = be.flatten()
        assert sp.contents.n_primitives == 1280 and sp.contents.bvh_reference_semantics == (2 if certified else 1)
        ctx.upload(sp)
        ctx.set_lens(0.35, 3.2, 0, 0.0)
        films[certified] = ctx.render(jp.render_params(24, 16, 16, 5, 31))
        assert ctx.build_info().certified_walk == (1 if certified else 0) and ctx.lens_info().lens_last_render == 1
    assert films[True].std() > 0.05 and _same(films[True], films[False])


# ---- G8 -------------------------------------------------------------------------------------------------------------------------------------------
def test_autofocus(ctx):
    depth = 7.5
    be = scenes.HostBackend("lens_focus_rect")
    be.camera(tuple(EYE), (0, 0, -1), (0, 1, 0), VFOV, W, Hh)
    be.rect(scenes.AXIS_XY, EYE[0] - 3.0, EYE[0] + 3.0, EYE[1] - 2.0, EYE[1] + 2.0, EYE[2] - depth, False, be.mat_matte((0.5, 0.5, 0.5)))
    be.preprocess()
    ctx.upload(be.flatten())
    for fx, fy in ((16.0, 12.0), (20.25, 9.5), (13.0, 17.75)):     # over the rectangle: the plane of focus through the hit is the rectangle's plane
        got = ctx.focus_distance(fx, fy)
        assert abs(got - depth) <= 4 * R.ulp32(depth), (fx, fy, got)
    assert ctx.focus_distance(1.0, 1.0) == 0.0                      # a miss
    # G3's emitter at that depth, focused by what its centre pixel sees: the pinhole's film away from the emitter's rim
    rho = 1.6
    be = _emitter(depth, rho)
    ctx.upload(be.flatten())
    focus = ctx.focus_distance(W / 2.0, Hh / 2.0)
    assert abs(focus - depth) <= 4 * R.ulp32(depth)
    p = jp.render_params(W, Hh, 64, 0, 5)
    pin = ctx.render(p)
    ctx.set_lens(1.0, focus, 0, 0.0)
    film = ctx.render(p)
    cam = be.flatten().contents.camera
    px = depth * np.linalg.norm(list(cam.up)) / Hh
    near, far = _box_distances(_focus_plane_boxes(cam, depth))
    interior = ~((far > rho - px) & (near < rho + px))             # a pixel of margin either side of the rim
    print("%d of %d pixels away from the rim; %d lit" % (interior.sum(), W * Hh, (pin[interior] > 0).sum()))
    assert interior.sum() > 0.8 * W * Hh and (pin[interior] > 0).sum() > 40
    assert _same(film[interior], pin[interior])                    # in focus: every lens ray of a pixel meets the emitter's plane where the pinhole ray does
    ctx.set_lens(1.0, 0.6 * focus, 0, 0.0)
    assert not _same(ctx.render(p)[interior], pin[interior])       # ... and out of focus it does not


# ---- G9 -------------------------------------------------------------------------------------------------------------------------------------------
def test_host_api_and_command_line(ctx, tmp_path):
    be = scenes.build_cornell(scenes.HostBackend("lens_host"), W, Hh, lambert_only=False)
    be.set_lens(14.0, 640.0, 7, 3.0)
    film = np.zeros((Hh, W, 3), f32); cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    assert be.last_focus() == 640.0
    ctx.upload(be.flatten())
    ctx.set_lens(14.0, 640.0, 7, 3.0)
    p = jp.render_params(W, Hh, 4, 5, 1234)
    direct = ctx.render(p)
    assert film.mean() > 0.05 and _same(film, direct)
    # FCamera::FocusAt
    be.set_lens(14.0, 1.0, 7, 3.0, focus_at=(16.0, 12.0))
    film2 = np.zeros((Hh, W, 3), f32)
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film2.ctypes.data, cnt) == 0
    found = ctx.focus_distance(16.0, 12.0)
    assert found > 100.0 and be.last_focus() == found
    ctx.set_lens(14.0, found, 7, 3.0)
    assert _same(film2, ctx.render(p))
    be.set_lens(0.0)                                               # ... and the pinhole again
    film3 = np.zeros((Hh, W, 3), f32)
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film3.ctypes.data, cnt) == 0
    ctx.set_lens(None)
    assert _same(film3, ctx.render(p))
    # jetpbrt --aperture R --focus-pixel X Y
    root = scenes.export_reference_layout(str(tmp_path / "scene"), 24, 16)
    out = str(tmp_path / "cornell")
    r = subprocess.run([jp.CLI_PATH, "0", "4", "32", "24", "--assets", root, "--out", out, "--aperture", "14", "--focus-pixel", "16", "12", "--blades", "7", "--aperture-rotation", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    m = re.search(r"lens: aperture 14, focus distance ([0-9.eE+-]+) \(found at the focus pixel\)", r.stderr)
    assert m, r.stderr
    hb = scenes.build_cornell(scenes.HostBackend("lens_cli"), 32, 24, lambert_only=False)
    ctx.upload(hb.flatten())
    want = ctx.focus_distance(16.0, 12.0)
    assert abs(float(m.group(1)) - want) <= 1e-5 * want             # (%g prints six digits)
    img = np.frombuffer(open(out + ".bmp", "rb").read()[54:], np.uint8).reshape(24, 32, 3)[::-1, :, ::-1]
    ctx.set_lens(14.0, want, 7, 3.0)
    assert np.array_equal(img, ctx.render_rgb8(jp.render_params(32, 24, 4, 5, 1234)))
    for bad in (["--aperture", "-1"], ["--aperture", "2", "--blades", "2"], ["--aperture", "2", "--focus", "0"]):
        r = subprocess.run([jp.CLI_PATH, "0", "1", "16", "16"] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 5, bad


# ---- G10 ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_lens_allocates_nothing(cornell):
    be, sp = cornell
    b0 = jp.device_bytes_in_use()
    c = jp.Context(0)
    try:
        c.upload(sp)
        p = jp.render_params(W, Hh, 4, 5, 1234)
        c.render(p); c.render_guides(p, 2)
        held = jp.device_bytes_in_use()
        c.set_lens(12.0, 700.0, 5, 0.0)
        assert jp.device_bytes_in_use() == held
        c.render(p); c.render_guides(p, 2)
        x, y, s = _pixels(W, Hh, 2)
        c.camera_rays(p, x, y, s); c.focus_distance(16.0, 12.0)
        assert jp.device_bytes_in_use() == held and c.lens_info().lens_last_render == 1
    finally:
        c.close()
    assert jp.device_bytes_in_use() == b0
