"""Interpolated shading normals on the MI355X (INTEGRATION.md "Vertex normals"): the hook against the host function bit for bit, all-flat normals are a
no-op, the deterministic direct light of a delta light per kernel family against the float64 predictor of tests/normals_ref.py, the geometric-side
guard, the map families against a quadrature of the texels, the guides, and the host API.  Figures these tests print are recorded in DESIGN.md
"Smooth normals"."""
import ctypes as C
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import denoise_ref as D
import envmap_ref as E
import mis_ref as M
import normals_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARGUMENT, UNSUPPORTED = -1, -5                             # JP_ERR_* of include/jetpbrt_amd.h
TAN_HALF = 0.75                                                   # |right| = |up| = 0.75: the film spans +-0.375 at unit distance


@pytest.fixture()
def ctx():
    """a context of its own per test: the normals, the map, the light sampling mode and the estimator are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _arr(ptr, n, k):
    return np.ctypeslib.as_array(ptr, (n * k,)).reshape(n, k).copy()


def _ico_asset(sub):
    p = os.path.join(scenes.asset_dir(), "normals_icosphere_%d.obj" % sub)
    v, f = R.icosphere(sub, 1.0, R.generic_rotation())
    return scenes.write_obj(p, v.astype(f32), f)


def _ico_scene(sub=1, size=48, light="dir", tex=False, env=None, mirror_light=False):
    """the icosphere at the origin seen from (0, -4, 0) along +y, up z, matte albedo 0.6 (or a checker of 0.6 / 0.3)"""
    be = scenes.HostBackend("normals_ico")
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), float(np.degrees(2.0 * np.arctan(TAN_HALF))), size, size)
    if light == "dir":
        wl = np.array([np.sin(np.radians(70.0)), -np.cos(np.radians(70.0)), 0.2]); wl /= np.linalg.norm(wl)
        be.dirlight(tuple(-wl), (3.0, 3.0, 3.0))                   # arriving from wl
    if env is not None:
        be.envlight(env)
    m = be.mat_matte(tex=be.texture_checker((0.6, 0.6, 0.6), (0.3, 0.3, 0.3))) if tex else be.mat_matte((0.6, 0.6, 0.6))
    be.mesh(_ico_asset(sub), False, False, mat=m)
    be.preprocess()
    return be


def _upload(ctx, be, vn, mode="all", tex=False, rgb=None, up="z"):
    ctx.set_environment_map(rgb, up)
    ctx.set_light_sampling(mode)
    ctx.set_vertex_normals(vn)
    ctx.upload(be.flatten(), be.flatten_textures() if tex else None)


# ---- 1. the hook, bit for bit ---------------------------------------------------------------------------------------------------------------------
def _tilted(ng, deg, rng, behind=False):
    out = []
    for _ in range(3):
        v = rng.normal(size=3); v -= (v @ ng) * ng; v /= np.linalg.norm(v)
        a = np.radians(rng.uniform(5, deg))
        n = np.cos(a) * ng + np.sin(a) * v
        out.append(-n if behind else n)
    return np.concatenate(out)


def _hook_scene(big):
    rng = np.random.default_rng(21)
    tris = [np.array([(-3.0, -1.0, 0.1), (-1.6, -0.8, -0.2), (-2.4, 0.9, 0.15)]), np.array([(-1.2, -1.0, 0.0), (0.2, -0.9, 0.1), (-0.5, 0.8, -0.1)]),
            np.array([(0.6, -1.0, 0.05), (2.0, -0.7, 0.0), (1.2, 0.9, 0.2)])]
    be = scenes.HostBackend("normals_hook")
    be.camera((0, 0, 8), (0, 0, -1), (0, 1, 0), 60.0, 16, 16)
    be.pointlight((0, 0, 6), (10, 10, 10))
    m = be.mat_matte((0.5, 0.5, 0.5))
    for k, t in enumerate(tris):
        p = os.path.join(scenes.asset_dir(), "normals_hook_tri_%d.obj" % k)
        be.mesh(scenes.write_obj(p, t.astype(f32), np.array([(0, 1, 2)])), False, False, mat=m)
    be.rect(scenes.AXIS_XY, 2.6, 3.8, -0.8, 0.8, 0.1, False, m)
    be.disk((-4.2, 0.0, 0.0), scenes._normalize((0.2, -0.3, 1.0)), 0.7, m)
    be.sphere((5.0, 0.0, 0.0), 0.8, m)
    if big:
        be.mesh(_ico_asset(3), False, False, offset=(0.0, 3.0, 0.0), mat=m)          # 1280 triangles: the 4-wide walk is under the hook
    be.preprocess()
    s = be.flatten().contents
    n = s.n_triangles
    p0, p1, p2, ng = (_arr(x, n, 3) for x in (s.tri_p0, s.tri_p1, s.tri_p2, s.tri_n))
    vn = np.zeros((n, 9), f32)
    small = []
    for t in range(n):
        if p0[t, 1] > 1.5:                                         # the icosphere: radial normals about its centre
            for k, p in enumerate((p0, p1, p2)):
                r = p[t].astype(np.float64) - (0.0, 3.0, 0.0)
                vn[t, 3 * k:3 * k + 3] = (r / np.linalg.norm(r)).astype(f32)
        else:
            small.append(t)
    small.sort(key=lambda t: p0[t, 0])
    vn[small[0]] = _tilted(ng[small[0]].astype(np.float64), 40.0, rng).astype(f32)                 # three distinct normals tilted up to 40 degrees
    vn[small[2]] = _tilted(ng[small[2]].astype(np.float64), 40.0, rng, behind=True).astype(f32)    # all behind Ng; small[1] stays flat
    return be, s, vn, (p0, p1, p2, ng), small


@pytest.mark.parametrize("big", [False, True])
def test_hook_is_the_host_function_bit_for_bit(ctx, big):
    be, s, vn, (p0, p1, p2, ng), small = _hook_scene(big)
    _upload(ctx, be, vn)
    info = ctx.normal_info()
    assert info.n_triangles == s.n_triangles and info.n_smooth_triangles == (2 + (1280 if big else 0)) and info.table_bytes_device == 48 * s.n_primitives
    if big:
        assert ctx.build_info().q4_nodes > 0
    rng = np.random.default_rng(5)
    n = 4096
    o = np.stack([rng.uniform(-5, 6, n), rng.uniform(-1.5, 4.5 if big else 1.5, n), np.full(n, 6.0)], -1)
    tgt = np.stack([rng.uniform(-5, 6, n), rng.uniform(-1.2, 4.2 if big else 1.2, n), np.zeros(n)], -1)
    d = tgt - o; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = o.astype(f32); d = d.astype(f32)
    t0 = np.full(n, 1e-3, f32); t1 = np.full(n, np.inf, f32)
    hit, t, prim_t, nrm_t = ctx.trace(o, d, t0, t1)
    prim, g, ns = ctx.shading_normal(o, d, t0, t1)
    assert np.array_equal(prim, prim_t) and _same(g, nrm_t)
    miss = prim < 0
    assert (g[miss] == 0).all() and (ns[miss] == 0).all()
    kind = np.array([s.prim_shape_type[i] for i in range(s.n_primitives)]); idx = np.array([s.prim_shape_index[i] for i in range(s.n_primitives)])
    tri = np.where(~miss & (kind[np.maximum(prim, 0)] == M.TRIANGLE), idx[np.maximum(prim, 0)], -1)
    smooth = (tri >= 0) & vn[np.maximum(tri, 0)].any(-1)
    other = ~miss & ~smooth
    print("hook (%s): %d rays, %d miss, %d on smooth triangles, %d on flat ones and other shapes; per small triangle %s" % (
        "big" if big else "tiny", n, miss.sum(), smooth.sum(), other.sum(), [int((tri == k).sum()) for k in small]))
    assert all((tri == k).sum() > 50 for k in small) and all((kind[prim[other]] == k).sum() > 50 for k in (1, 2, 3))
    assert _same(ns[other], g[other])
    k = tri[smooth]
    p = (o[smooth] + t[smooth, None] * d[smooth]).astype(f32)      # ray(distance) as the kernels form it: one fp32 multiply and add per component
    want = jp.interpolate_normals(p0[k], p1[k], p2[k], ng[k], vn[k], p)
    assert _same(ns[smooth], want)
    assert ((ns[smooth] * g[smooth]).sum(-1) >= 0).all()
    assert (ns[smooth] != g[smooth]).any(-1).mean() > 0.99


# ---- 2. all-flat normals are a no-op ---------------------------------------------------------------------------------------------------------------
def test_flat_normals_change_nothing():
    start = jp.device_bytes_in_use()
    W, H = 64, 48
    be = scenes.build_cornell(scenes.HostBackend("normals_noop"), W, H, lambert_only=False)
    s = be.flatten().contents
    rp = jp.render_params(W, H, 4, 5, 99)
    c = jp.Context(0)
    try:
        c.upload(be.flatten())
        film0 = c.render(rp); g0 = c.render_guides(rp, 3)
        assert c.normal_info().smooth_last_render == 0 and c.normal_info().n_triangles == 0
        c.set_vertex_normals(np.zeros((s.n_triangles, 9), f32))
        c.upload(be.flatten())
        film1 = c.render(rp); g1 = c.render_guides(rp, 3)
        i = c.normal_info()
        assert i.smooth_last_render == 0 and i.n_triangles == s.n_triangles and i.n_smooth_triangles == 0 and i.table_bytes_device == 0
        assert _same(film0, film1) and all(_same(a, b) for a, b in zip(g0, g1))
        # a count that differs from the scene's is refused, and the context stays usable
        c.set_vertex_normals(np.zeros((s.n_triangles + 1, 9), f32))
        with pytest.raises(jp.JetPbrtError) as e:
            c.upload(be.flatten())
        assert "status %d" % INVALID_ARGUMENT in str(e.value) and "n_triangles" in str(e.value)
        c.set_vertex_normals(None)
        c.upload(be.flatten())
        assert _same(c.render(rp), film0)
    finally:
        c.close()
    assert jp.device_bytes_in_use() == start


# ---- 3. deterministic direct light, per family ------------------------------------------------------------------------------------------------------
FAMILIES = {"all": dict(mode="all", est="nee", tex=False), "power": dict(mode="power", est="nee", tex=False),
            "mis": dict(mode="power", est="mis", tex=False), "textured": dict(mode="all", est="nee", tex=True)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_direct_light_of_a_delta_light_equals_the_predictor(ctx, family):
    """Film of the smooth 80-triangle icosphere under one directional light, max_depth 1, debug sampler: within 1e-5 absolute of the float64 predictor on
    every hit pixel the predictor does not mark fragile (at most 2 % of the hit pixels)."""
    fam = FAMILIES[family]
    be = _ico_scene(1, 48, tex=fam["tex"])
    s = be.flatten().contents
    vn = R.radial_normals(s)
    _upload(ctx, be, vn, fam["mode"], fam["tex"])
    ctx.set_estimator(fam["est"])
    rp = jp.render_params(48, 48, 1, 1, 7, sampler_mode=jp.JP_SAMPLER_DEBUG)
    film = ctx.render(rp)
    assert ctx.normal_info().smooth_last_render == 1 and ctx.normal_info().n_smooth_triangles == 80
    o, d = R.camera_rays(s)
    _, _, alb = ctx.surface(o.astype(f32), d.astype(f32), np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32))
    pred, hit, fragile, n_only, g_only = R.direct_delta(s, vn, alb)
    flat, _, _, _, _ = R.direct_delta(s, vn, alb, use_ng=True)
    keep = hit & ~fragile
    err = np.abs(film.astype(np.float64) - pred).max(-1)
    print("%s: %d hit pixels, %d fragile, %d lit by Ns and blacked by the guard, %d the other way round; mean |flat - smooth| %.4f; largest error %.3e (kept), %.3e (fragile)" % (
        family, hit.sum(), fragile.sum(), n_only.sum(), g_only.sum(), np.abs(flat - pred).max(-1)[hit].mean(), err[keep].max(), err[hit & fragile].max() if (hit & fragile).any() else 0.0))
    assert hit.sum() > 700 and fragile.sum() <= 0.02 * hit.sum()
    assert (film[~hit] == 0).all()
    assert err[keep].max() <= 1e-5
    assert np.abs(film.astype(np.float64) - flat).max(-1)[hit].mean() > 0.01      # a flat render is far off


# ---- 4. the guard ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [False, True])
def test_guard_blacks_a_light_below_the_geometric_plane(ctx, above):
    """one triangle in the plane z = 0 with normals tilted 40 degrees toward +x; a point light below the geometric plane but above the shading plane gives
    exactly 0, the light mirrored above the plane gives the predictor's value"""
    be = scenes.HostBackend("normals_guard")
    be.camera((0, 0, 4), (0, 0, -1), (0, 1, 0), 30.0, 1, 1)
    lz = 0.3 if above else -0.3
    be.pointlight((3.0, 0.0, lz), (20.0, 20.0, 20.0))
    m = be.mat_matte((0.6, 0.6, 0.6))
    p = os.path.join(scenes.asset_dir(), "normals_guard_tri.obj")
    be.mesh(scenes.write_obj(p, np.array([(-2, -2, 0), (2, -2, 0), (0, 3, 0)], f32), np.array([(0, 1, 2)])), False, False, mat=m)
    be.preprocess()
    a = np.radians(40.0)
    n = np.array([np.sin(a), 0.0, np.cos(a)])
    vn = np.tile(n, 3)[None].astype(f32)
    _upload(ctx, be, vn)
    film = ctx.render(jp.render_params(1, 1, 1, 1, 3, sampler_mode=jp.JP_SAMPLER_DEBUG))
    assert ctx.normal_info().smooth_last_render == 1
    # the pixel-centre ray hits the origin; Ns there is n up to fp32 rounding
    wi = np.array([3.0, 0.0, lz]); d2 = wi @ wi; wi /= np.sqrt(d2)
    nf = vn[0, :3].astype(np.float64); nf /= np.linalg.norm(nf)
    assert wi @ nf > 0.3 and (wi[2] > 0) == above                   # above the shading plane either way; below the geometric plane unless mirrored
    want = 0.6 / np.pi * (20.0 / d2) * abs(wi @ nf) if above else 0.0
    print("guard (%s the plane): film %r, predicted %.7f" % ("above" if above else "below", film[0, 0].tolist(), want))
    if above:
        assert np.abs(film[0, 0].astype(np.float64) - want).max() <= 1e-5 and want > 0.1
    else:
        assert (film[0, 0] == 0).all()


# ---- 5. the map families -----------------------------------------------------------------------------------------------------------------------------
TINT = (0.05, 0.05, 0.05)                                        # the scene's environment light tints the map: the film stays below the clamp at 1


def _map():
    rgb = np.full((4, 8, 3), 0.05, f32)
    rgb[1, 6] = 40.0                                               # from the camera's side, above the horizon
    return rgb


MAP_SEEDS, MAP_SPP, MAP_SIZE = tuple(range(1000, 1008)), 64, 32
_map_ref = {}


def _map_reference(s, vn):
    """the quadrature of tests/normals_ref.py at the very camera rays the 8 x 64 samples of a pixel take (the counter sampler jitters them inside the
    pixel), computed once for the three families: per ray the hit, the irradiance-like integrals with Ns and with Ng, the texel a miss sees"""
    if not _map_ref:
        rays = [D.camera_rays(s.camera, MAP_SIZE, MAP_SIZE, seed, k) for seed in MAP_SEEDS for k in range(MAP_SPP)]
        o = np.concatenate([r[0] for r in rays]); d = np.concatenate([r[1] for r in rays])
        _map_ref["rays"] = (o, d)
        _map_ref["ref"] = R.map_direct_rays(s, vn, o, d, _map(), TINT, E.UP_Z, through_camera=True)
    return _map_ref["rays"], _map_ref["ref"]


@pytest.mark.parametrize("family", ["map", "map_mis", "map_textured"])
def test_map_families_match_the_texel_quadrature(ctx, family):
    """The icosphere under an 8 x 4 map with one bright texel, POWER_ONE, max_depth 1, 32 x 32: the mean of 8 seeds of 64 spp against the float64
    quadrature of the direct light over every texel; |mean - predicted| <= 5 se + 1e-3 on all but 1 % of the hit pixels, and the same quadrature with
    Ng in place of Ns must fail that on at least 20 % of the lit pixels."""
    tex = family == "map_textured"
    rgb = _map()
    be = _ico_scene(1, 32, light=None, tex=tex, env=TINT)
    s = be.flatten().contents
    vn = R.radial_normals(s)
    _upload(ctx, be, vn, "power", tex, rgb, "z")
    ctx.set_estimator("mis" if family == "map_mis" else "nee")
    films = np.stack([ctx.render(jp.render_params(MAP_SIZE, MAP_SIZE, MAP_SPP, 1, seed)).astype(np.float64) for seed in MAP_SEEDS])
    assert ctx.normal_info().smooth_last_render == 1 and ctx.env_info().mapped_last_render == 1
    (o, d), (hit_r, E_ns, E_ng, miss) = _map_reference(s, vn)
    _, _, alb = ctx.surface(o, d, np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32))
    per_pixel = lambda E_: np.where(hit_r[:, None], alb.astype(np.float64) / np.pi * E_, miss).reshape(len(MAP_SEEDS) * MAP_SPP, MAP_SIZE, MAP_SIZE, 3).mean(0)
    pred, flat = per_pixel(E_ns), per_pixel(E_ng)
    hit = hit_r.reshape(-1, MAP_SIZE, MAP_SIZE).all(0)             # every sample of the pixel hits the mesh (the others: compared all the same, as "not hit")
    mean = films.mean(0); se = films.std(0, ddof=1) / np.sqrt(8.0)
    assert films.max() < 1.0 and pred.max() < 1.0                  # nothing near the film's clamp
    bad = (np.abs(mean - pred) > 5.0 * se + 1e-3).any(-1)
    lit = hit & (pred.max(-1) > 0.01)                              # lit by the bright texel (the rest of the map gives 0.0015 at most)
    bad_flat = (np.abs(mean - flat) > 5.0 * se + 1e-3).any(-1) & lit
    print("%s: %d hit pixels, %d outside 5 se + 1e-3 (largest |mean - predicted| %.3e, largest se %.3e); with Ng in place of Ns %d of %d lit pixels outside" % (
        family, hit.sum(), bad.sum(), np.abs(mean - pred)[hit].max(), se[hit].max(), bad_flat.sum(), lit.sum()))
    assert hit.sum() > 300 and lit.sum() > 100
    assert bad.sum() <= 0.01 * hit.sum()                           # (silhouette and background pixels included in the count)
    assert bad_flat.sum() >= 0.2 * lit.sum()


# ---- 6. the guides ---------------------------------------------------------------------------------------------------------------------------------
def test_normal_guide_is_the_shading_normal(ctx):
    be = _ico_scene(1, 48)
    s = be.flatten().contents
    vn = R.radial_normals(s)
    rp = jp.render_params(48, 48, 1, 1, 11)
    _upload(ctx, be, None)
    flat = ctx.render_guides(rp, 3)
    _upload(ctx, be, vn)
    alb, nrm, dep = ctx.render_guides(rp, 3)
    N = np.zeros((48 * 48, 3), f32); NG = np.zeros((48 * 48, 3), f32)
    for k in range(3):
        o, d, t0, t1 = D.camera_rays(s.camera, 48, 48, 11, k)
        prim, g, ns = ctx.shading_normal(o, d, t0, t1)
        N = (N + ns).astype(f32); NG = (NG + g).astype(f32)
    inv = f32(1.0) / f32(3)
    assert _same(nrm, (N * inv).astype(f32).reshape(48, 48, 3))
    assert _same(flat[1], (NG * inv).astype(f32).reshape(48, 48, 3))        # the guide of the flat upload: as ever
    assert _same(alb, flat[0]) and _same(dep, flat[2])
    hitm = dep > 0
    assert (nrm[hitm] != flat[1][hitm]).any(-1).mean() > 0.95


# ---- 7. host API, Whitted --------------------------------------------------------------------------------------------------------------------------
def test_host_render_equals_the_c_abi_render(ctx):
    v, f = R.icosphere(1, 1.0, R.generic_rotation())
    path = scenes.write_obj(os.path.join(scenes.asset_dir(), "normals_ico_vn.obj"), v.astype(f32), f, normals=(v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32))

    def build(smooth):
        be = scenes.HostBackend("normals_host_api")
        be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), 40.0, 32, 32)
        be.pointlight((3.0, -3.0, 2.0), (30.0, 30.0, 30.0))
        be.mesh(path, False, False, mat=be.mat_plastic((0.5, 0.3, 0.2), (0.3, 0.3, 0.3), 0.1), smooth=smooth)
        be.preprocess()
        return be
    be = build("file")
    film = np.zeros((32, 32, 3), f32)
    cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, 32, 32, 4, 3, 77, 0, 0, 1, film.ctypes.data, cnt) == 0
    vn = be.flatten_normals()
    assert vn is not None and vn.n_triangles == 80
    _upload(ctx, be, vn)
    got = ctx.render(jp.render_params(32, 32, 4, 3, 77))
    assert ctx.normal_info().smooth_last_render == 1 and ctx.normal_info().n_smooth_triangles == 80
    assert _same(film, got) and film.mean() > 0.01
    flat_be = build(None)                                          # the default stays flat although the file has vn
    assert flat_be.flatten_normals() is None
    film_flat = np.zeros((32, 32, 3), f32)
    assert jp.host_lib().jp_host_render(flat_be.h, 32, 32, 4, 3, 77, 0, 0, 1, film_flat.ctypes.data, cnt) == 0
    assert not _same(film, film_flat)


def test_whitted_refuses_a_smooth_scene_and_the_context_survives(ctx):
    be = _ico_scene(1, 32)
    s = be.flatten().contents
    _upload(ctx, be, R.radial_normals(s))
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.render(jp.render_params(32, 32, 1, 3, 5, integrator=jp.JP_INTEGRATOR_WHITTED))
    assert "status %d" % UNSUPPORTED in str(e.value)
    dbg = ctx.render(jp.render_params(32, 32, 1, 3, 5, integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))     # ignores the normals
    assert ctx.normal_info().smooth_last_render == 0
    film = ctx.render(jp.render_params(32, 32, 2, 3, 5))
    assert ctx.normal_info().smooth_last_render == 1 and film.mean() > 0.005 and np.isfinite(dbg).all()
    # refusals of jp_set_vertex_normals leave the state alone
    bad = R.radial_normals(s); bad[3, 4] = np.nan
    with pytest.raises(jp.JetPbrtError):
        ctx.set_vertex_normals(bad)
    ctx.upload(be.flatten())
    assert ctx.normal_info().n_smooth_triangles == 80
