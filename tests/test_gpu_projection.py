"""Camera projections on the MI355X (INTEGRATION.md "Projections"): the hook against the host function bit for bit, no projection is a no-op, the film of an
emitter against jp_trace over the hooked rays exactly, orthographic films do not depend on depth, a panorama of an environment map is the map, guides and the
other integrators, the refusals, the certified walk, adaptive sampling, device memory.  Films are at most 48 x 32 at <= 16 spp."""
import ctypes as C
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import projection_ref as R
import normals_ref as NR

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARGUMENT, UNSUPPORTED = -1, -5
W, Hh = 32, 24
EYE = np.array([10.0, -4.0, 30.0])                                # the emitter scenes' camera: looks along -z, up +y; |up| = tan(45 deg) = 1, |right| = 4 / 3
VFOV = 90.0
# per kind: the projection and the emitter (offset from the camera's axis, radius) of G3 / G4 at depth 3 -- off-centre in every frame
ORTHO = dict(kind=R.ORTHOGRAPHIC, ortho_scale=6.0)                 # the view is 8 x 6 scene units
EQUIRECT = dict(kind=R.EQUIRECT)
FISHEYE = dict(kind=R.FISHEYE, fov_deg=180.0, fit=R.FIT_DIAGONAL)
KINDS = [("ortho", ORTHO, (1.5, -0.8, 1.5)), ("equirect", EQUIRECT, (2.0, -1.0, 3.0)), ("fisheye", FISHEYE, (2.0, -1.0, 3.0))]
IDS = [k[0] for k in KINDS]


@pytest.fixture()
def ctx():
    """a context of its own per test: the projection is context state"""
    c = jp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell():
    be = scenes.build_cornell(scenes.HostBackend("projection_cornell"), W, Hh, lambert_only=False)
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


def _emitter(z, off):
    """one emissive disk facing the camera at depth z, its centre (dx, dy) off the camera's axis, radiance (1, 1, 1), a black material; nothing else, no background"""
    dx, dy, rho = off
    be = scenes.HostBackend("projection_emitter")
    be.camera(tuple(EYE), (0, 0, -1), (0, 1, 0), VFOV, W, Hh)
    be.disk((EYE[0] + dx, EYE[1] + dy, EYE[2] - z), (0, 0, 1), rho, be.mat_matte((0.0, 0.0, 0.0)), (1.0, 1.0, 1.0))
    be.preprocess()
    return be


# ---- G1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,_", KINDS, ids=IDS)
def test_hook_is_the_host_function(ctx, cornell, name, kw, _):
    be, sp = cornell
    ctx.upload(sp)
    cam = sp.contents.camera
    rng = np.random.default_rng(9)
    n = 5000
    x = rng.integers(0, W, n).astype(np.int32); y = rng.integers(0, Hh, n).astype(np.int32); s = rng.integers(0, 4096, n).astype(np.int32)
    p = jp.render_params(W, Hh, 1, 5, 4242)
    proj = jp.projection(**kw) if name != "ortho" else jp.projection(R.ORTHOGRAPHIC, 400.0)
    ctx.set_projection(proj)
    exact = name == "ortho" or ctx.build_info().libm_sincosf != 0
    for debug in (False, True):
        pp = jp.render_params(W, Hh, 1, 5, 4242, sampler_mode=jp.JP_SAMPLER_DEBUG) if debug else p
        o, d, k = ctx.camera_rays(pp, x, y, s)
        fxfy = R.sample_draws(4242, x, y, s, debug=debug)
        ho, hd = jp.projection_rays(cam, proj, fxfy)
        assert (k == 2).all()                                      # no new draws: the first bounce draws from dim 2
        assert _same(o, ho)
        if exact:
            assert _same(d, hd)
        else:                                                      # a host libm the device does not reproduce: sine / cosine may differ in the last place
            err = np.abs(d - hd).max()
            print("%s: largest direction difference %.3e" % (name, err))
            assert err <= 1e-6
        ro, rd = R.rays(cam, fxfy=fxfy, **({"kind": proj.kind, "ortho_scale": proj.ortho_scale, "fov_deg": proj.fov_deg, "fit": proj.fit}))
        assert np.abs(d - rd).max() <= 1e-5                        # ... and both are the mapping (test_projection_host.py's bound)
    if name == "ortho":
        assert np.abs(o - np.array(list(cam.pos), f32)).max() > 50.0 and (d.view(np.uint32) == d[0].view(np.uint32)[None]).all()
    else:
        assert (o == np.array(list(cam.pos), f32)[None]).all()
    info = ctx.projection_info()
    assert (info.kind, info.ortho_scale, info.fov_deg, info.fit) == (proj.kind, proj.ortho_scale, proj.fov_deg, proj.fit)
    ctx.set_projection(None)                                        # ... and the pinhole again
    o0, d0, k0 = ctx.camera_rays(p, x, y, s)
    ho, hd = jp.projection_rays(cam, None, R.sample_draws(4242, x, y, s))
    assert (k0 == 2).all() and _same(o0, ho) and _same(d0, hd)


# ---- G2 -------------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(ctx, cornell):
    be, sp = cornell
    ctx.upload(sp)
    p = jp.render_params(W, Hh, 8, 5, 1234)

    def shot():
        film = ctx.render(p); c = ctx.counters()
        i = ctx.projection_info()
        assert i.projected_last_render == 0 and i.gamma0_last_render == 0.0 and i.kind == 0
        return film, (c.samples, c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded), ctx.render_guides(p, 2)
    base = shot()
    ctx.set_projection(None); null = shot()
    ctx.set_projection(jp.projection(R.PERSPECTIVE, 3.0, 90.0, R.FIT_WIDTH)); zero = shot()
    ctx.set_projection("equirect"); film_on = ctx.render(p)
    assert ctx.projection_info().projected_last_render == 1 and not _same(film_on, base[0])
    assert not _same(ctx.render_guides(p, 2)[2], base[2][2])
    ctx.set_projection(None); back = shot()
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


@pytest.mark.parametrize("name,kw,off", KINDS, ids=IDS)
def test_film_is_made_of_the_hooked_rays(ctx, name, kw, off):
    be = _emitter(3.0, off)                                        # (kept alive: the flattened scene is the backend's memory)
    ctx.upload(be.flatten())
    p = jp.render_params(W, Hh, 8, 0, 99)                          # max_depth 0: a path is its first hit's emission, 1 or 0
    pin = ctx.render(p)
    assert _same(pin, _film_from_hooked_rays(ctx, p))
    ctx.set_projection(jp.projection(**kw))
    film = ctx.render(p)
    assert ctx.projection_info().projected_last_render == 1 and ctx.build_info().fused_last_render == 0
    want = _film_from_hooked_rays(ctx, p)
    seen = (film[..., 0] > 0).mean()
    ys, xs = np.nonzero(film[..., 0] > 0)
    print("%s: %.1f %% of the pixels see the disk, centred on (%.1f, %.1f) of %d x %d" % (name, 100 * seen, xs.mean(), ys.mean(), W, Hh))
    assert 0.05 <= seen <= 0.60                                    # a blank film cannot pass
    assert xs.mean() < (W - 1) / 2 - 1 and ys.mean() > (Hh - 1) / 2 + 1      # off-centre: to the left of (the camera's right = up x front is -x) and below the middle
    assert _same(film, want) and not _same(film, pin)
    assert set(np.unique(film * 8)) <= set(range(9))
    # two lanes, and the fused option (falls back to the per-bounce launches): the same film
    ctx.set_options(lanes=2)
    assert _same(ctx.render(p), want) and ctx.build_info().lanes_last_render == 2
    ctx.set_options(); ctx.set_options(fused=1)
    assert _same(ctx.render(p), want) and ctx.build_info().fused_last_render == 0 and ctx.projection_info().projected_last_render == 1
    ctx.set_options()


# ---- G4 -------------------------------------------------------------------------------------------------------------------------------------------
def test_orthographic_means_no_perspective(ctx):
    films = {}
    for z in (3.0, 6.0):
        be = _emitter(z, KINDS[0][2])
        ctx.upload(be.flatten())
        p = jp.render_params(W, Hh, 8, 0, 99)
        ctx.set_projection(None); pin = ctx.render(p)
        ctx.set_projection(jp.projection(**ORTHO)); films[z] = (pin, ctx.render(p))
    assert 0.05 <= (films[3.0][1] > 0).mean() <= 0.60
    assert _same(films[3.0][1], films[6.0][1])
    assert not _same(films[3.0][0], films[6.0][0]) and films[6.0][0].sum() < 0.5 * films[3.0][0].sum()


# ---- G5 -------------------------------------------------------------------------------------------------------------------------------------------
EW, EH = 32, 16


def _probe_scene(ctx, rgb):
    """a small sphere and an environment light around a camera at the origin whose axes are the ones INTEGRATION.md prescribes for JP_ENV_UP_Z:
    front = -x, up = +z, and with them FCamera's right = up x front = -y (the map's azimuth grows to the left of a viewer inside it)"""
    be = scenes.HostBackend("projection_probe")
    be.camera((0, 0, 0), (-1, 0, 0), (0, 0, 1), 90.0, EW, EH)
    be.envlight((1.0, 1.0, 1.0))
    be.sphere((-3.0, 0.4, 0.3), 0.8, be.mat_matte((0.5, 0.5, 0.5)))
    be.preprocess()
    sc = jp.JpScene.from_buffer_copy(be.flatten().contents)
    assert np.allclose(np.array(list(sc.camera.right)) / np.linalg.norm(list(sc.camera.right)), [0.0, -1.0, 0.0], atol=1e-6)
    ctx.set_environment_map(rgb, "z"); ctx.set_light_sampling("power")
    ctx.upload(C.pointer(sc))
    return be, sc


@pytest.mark.parametrize("name,kw", [("equirect", EQUIRECT), ("fisheye", FISHEYE), ("ortho", dict(kind=R.ORTHOGRAPHIC, ortho_scale=4.0))])
def test_a_panorama_of_an_environment_map_is_the_map(ctx, name, kw):
    rgb = np.random.default_rng(5).uniform(0.05, 4.0, (EH, EW, 3)).astype(f32)
    be, sc = _probe_scene(ctx, rgb)
    ctx.set_film(1); ctx.set_projection(jp.projection(**kw))
    p = jp.render_params(EW, EH, 1, 5, 7, sampler_mode=jp.JP_SAMPLER_DEBUG)
    film = ctx.render(p)
    assert ctx.projection_info().projected_last_render == 1
    x, y, s = _pixels(EW, EH, 1)
    o, d, _ = ctx.camera_rays(p, x, y, s)
    miss = _trace_all(ctx, o, d)[0] == 0
    idx, lrgb = ctx.env_lookup(d)
    print("%s: %d of %d pixels miss the sphere" % (name, miss.sum(), miss.size))
    assert miss.mean() >= 0.80 and (~miss).sum() >= 1
    assert _same(film.reshape(-1, 3)[miss], lrgb[miss])
    if name == "equirect":
        own = idx == (y * EW + x)
        print("equirect: %d of the %d miss pixels see their own texel; %d see a neighbour (rounding at a texel edge)" % (own[miss].sum(), miss.sum(), (~own[miss]).sum()))
        assert own[miss].mean() >= 0.95
        assert _same(film.reshape(-1, 3)[miss & own], rgb.reshape(-1, 3)[miss & own])     # the film is the map
    else:
        n_texels = len(np.unique(idx[miss]))
        assert n_texels == 1 if name == "ortho" else n_texels >= 50                     # (orthographic: one direction, one texel)


# ---- G6 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,_", KINDS, ids=IDS)
def test_guides(ctx, cornell, name, kw, _):
    be, sp = cornell
    ctx.upload(sp)
    proj = jp.projection(**kw) if name != "ortho" else jp.projection(R.ORTHOGRAPHIC, 500.0)
    ctx.set_projection(proj)
    spp = 2
    p = jp.render_params(W, Hh, spp, 5, 808, sampler_mode=jp.JP_SAMPLER_DEBUG)
    x, y, s = _pixels(W, Hh, spp)
    o, d, _ = ctx.camera_rays(p, x, y, s)
    hit, t, prim, nrm = _trace_all(ctx, o, d)
    assert 0 < hit.sum() and len(np.unique(prim[hit > 0])) >= 2
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
    ctx.set_projection(None)
    assert not _same(ctx.render_guides(p, spp)[2], gz)


def test_the_other_integrators(ctx, cornell):
    be, sp = cornell
    ctx.upload(sp)
    ctx.set_projection("equirect")
    spp = 4
    pn = jp.render_params(W, Hh, spp, 5, 808, integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL)
    x, y, s = _pixels(W, Hh, spp)
    o, d, _ = ctx.camera_rays(pn, x, y, s)
    hit, t, prim, nrm = _trace_all(ctx, o, d)
    nn = np.where(hit[:, None] > 0, nrm, f32(0)).astype(f32).reshape(-1, spp, 3)
    # the debug-normal integrator: the same rays, the normal as a colour, k_resolve's sum
    film = ctx.render(pn)
    assert ctx.projection_info().projected_last_render == 1 and hit.sum() > 0
    assert _same(film.reshape(-1, 3), _resolve(nn, spp))
    gn = ctx.render_guides(pn, spp)[1]                             # ... which is the guide's normal, clamped as the film is
    assert np.abs(film - np.clip(gn, 0.0, 1.0)).max() <= 4 * 2.0 ** -24
    pw = jp.render_params(W, Hh, spp, 5, 808, integrator=jp.JP_INTEGRATOR_WHITTED)
    fw = ctx.render(pw)
    assert np.isfinite(fw).all() and fw.max() > 0.05 and ctx.projection_info().projected_last_render == 1
    ctx.set_projection(None)
    assert not _same(ctx.render(pw), fw)


# ---- G7 -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(ctx, cornell):
    be, sp = cornell
    ctx.upload(sp)
    p = jp.render_params(W, Hh, 4, 5, 1234)
    base = ctx.render(p)
    film = np.zeros((Hh, W, 3), f32); q = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.set_lens(12.0, 700.0); ctx.set_projection("equirect")
    assert ctx.lib.jp_render(ctx.h, C.byref(p), q(film)) == UNSUPPORTED and "lens" in ctx.lib.jp_last_error().decode()
    for call in (lambda: ctx.render_guides(p, 2), lambda: ctx.render_adaptive(jp.render_params(W, Hh, 16, 5, 1234), jp.adaptive(0.2, 8, 8, 16)), lambda: ctx.camera_rays(p, [0], [0], [0])):
        with pytest.raises(jp.JetPbrtError, match="status -5.*lens"):
            call()
    assert ctx.projection_info().projected_last_render == 0
    ctx.set_lens(None); ctx.set_projection(None)
    assert _same(ctx.render(p), base)                              # the context stays usable
    # a bad projection is refused when it is set, and the one in force stays
    ctx.set_projection("fisheye", fov_deg=200.0, fit="height")
    for bad, word in ((jp.projection(5), "kind"), (jp.projection(R.ORTHOGRAPHIC, -1.0), "ortho_scale"), (jp.projection(R.FISHEYE, 0.0, 400.0), "fov_deg"), (jp.projection(R.FISHEYE, 0.0, 90.0, 4), "fit")):
        assert ctx.lib.jp_set_projection(ctx.h, C.byref(bad)) == INVALID_ARGUMENT and word in ctx.lib.jp_last_error().decode()
    i = ctx.projection_info()
    assert (i.kind, i.ortho_scale, i.fov_deg, i.fit, i.projected_last_render) == (R.FISHEYE, 0.0, 200.0, R.FIT_HEIGHT, 0)
    cam = sp.contents.camera
    ctx.render(p)
    i = ctx.projection_info()
    assert i.projected_last_render == 1 and i.gamma0_last_render == R.gamma0(cam, R.FISHEYE, 200.0, R.FIT_HEIGHT) and i.gamma0_last_render > 0
    ctx.set_projection("equirect"); ctx.render(p)
    assert ctx.projection_info().gamma0_last_render == f32(f32(np.pi) / f32(Hh))
    ctx.set_projection("ortho", ortho_scale=300.0); ctx.render(p)
    i = ctx.projection_info()
    assert (i.kind, i.ortho_scale, i.projected_last_render, i.gamma0_last_render) == (R.ORTHOGRAPHIC, 300.0, 1, 0.0)
    # a camera whose axes are not perpendicular: refused at render time for a panorama, the context stays usable
    sc = jp.JpScene.from_buffer_copy(sp.contents)
    sc.camera.up[0] = 0.3 * sc.camera.up[1]
    ctx.upload(C.pointer(sc)); ctx.set_projection("equirect")
    assert ctx.lib.jp_render(ctx.h, C.byref(p), q(film)) == INVALID_ARGUMENT and "perpendicular" in ctx.lib.jp_last_error().decode()
    ctx.set_projection("ortho", ortho_scale=300.0)
    assert ctx.render(p).mean() > 0.01


def _ico_scene(certified):
    p = os.path.join(scenes.asset_dir(), "projection_icosphere_3.obj")
    v, f = NR.icosphere(3, 1.0, NR.generic_rotation())
    be = scenes.HostBackend("projection_ico")
    be.set_reference_tree(True, certified=certified)
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), 40.0, 24, 16)
    be.envlight((0.4, 0.5, 0.7))
    be.pointlight((3.0, -3.0, 4.0), (30.0, 30.0, 30.0))
    be.mesh(scenes.write_obj(p, v.astype(f32), f), False, False, mat=be.mat_matte((0.6, 0.6, 0.6)))
    be.preprocess()
    return be


def test_certified_walk_with_an_orthographic_camera(ctx):
    films = {}
    for certified in (False, True):
        be = _ico_scene(certified)
        sp = be.flatten()
        assert sp.contents.n_primitives == 1280 and sp.contents.bvh_reference_semantics == (2 if certified else 1)
        ctx.upload(sp)
        ctx.set_projection("ortho", ortho_scale=6.0)
        films[certified] = ctx.render(jp.render_params(24, 16, 16, 5, 31))
        assert ctx.build_info().certified_walk == (1 if certified else 0) and ctx.projection_info().projected_last_render == 1
    assert films[True].std() > 0.05 and _same(films[True], films[False])


def test_adaptive_under_a_fisheye(ctx):
    """every pixel of an adaptive render equals the uniform render of its own sample count (k_raygen_list_proj), as test_gpu_adaptive.py has it for the pinhole"""
    w, h, MIN, STEP, MAX, THR = 40, 24, 8, 8, 16, 0.2
    be = scenes.build_cornell(scenes.HostBackend("projection_adaptive"), w, h, lambert_only=False)
    ctx.upload(be.flatten())
    ctx.set_projection("fisheye", fov_deg=100.0)
    rp = jp.render_params(w, h, MAX, 5, 1234)
    film, counts, var = ctx.render_adaptive(rp, jp.adaptive(THR, MIN, STEP, MAX, 0.0, 1))
    i = ctx.projection_info()
    assert i.projected_last_render == 1 and i.gamma0_last_render > 0
    values, share = np.unique(counts, return_counts=True)
    print("fisheye: counts %s, pixels %s" % (values.tolist(), share.tolist()))
    assert set(values) == {8, 16} and (share >= 0.05 * counts.size).all()      # the scene adapts
    uniform = {}
    for n in values:
        f, k, v = ctx.render_adaptive(rp, jp.adaptive(THR, int(n), STEP, int(n), 0.0, 1))
        m = counts == n
        assert (k == n).all() and _same(film[m], f[m]) and _same(var[m], v[m])
        uniform[int(n)] = f
    ctx.set_projection(None)
    assert not _same(ctx.render_adaptive(rp, jp.adaptive(THR, 8, STEP, 8, 0.0, 1))[0], uniform[8])


def test_a_projection_allocates_nothing(cornell):
    be, sp = cornell
    b0 = jp.device_bytes_in_use()
    c = jp.Context(0)
    try:
        c.upload(sp)
        p = jp.render_params(W, Hh, 4, 5, 1234)
        c.render(p); c.render_guides(p, 2)
        x, y, s = _pixels(W, Hh, 2)
        c.camera_rays(p, x, y, s)
        held = jp.device_bytes_in_use()
        for kind in ("ortho", "equirect", "fisheye"):
            c.set_projection(kind)
            assert jp.device_bytes_in_use() == held
            c.render(p); c.render_guides(p, 2); c.camera_rays(p, x, y, s)
            assert jp.device_bytes_in_use() == held and c.projection_info().projected_last_render == 1
    finally:
        c.close()
    assert jp.device_bytes_in_use() == b0
