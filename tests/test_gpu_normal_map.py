"""Normal maps on the MI355X (INTEGRATION.md "Normal maps"): the hook against the host function bit for bit on triangles and rectangles and within the
host test's angle bound on spheres and disks, neutral and absent maps are a no-op, the deterministic direct light of a delta light per kernel family
against the float64 predictor of tests/normal_map_ref.py, the geometric-side guard, the map families against the quadrature of the texels, the guides, and the refusals and fallbacks.  Figures these tests
print are recorded in DESIGN.md "Normal maps"."""
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import denoise_ref as D
import envmap_ref as E
import mis_ref as M
import normals_ref as NR
import normal_map_ref as R
from test_normal_map_host import ANGLE_BOUND

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARGUMENT, UNSUPPORTED = -1, -5                             # JP_ERR_* of include/jetpbrt_amd.h
TAN_HALF = 0.75


@pytest.fixture()
def ctx():
    """a context of its own per test: the maps, the normals, the light sampling mode and the estimator are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _arr(ptr, n, k):
    return np.ctypeslib.as_array(ptr, (n * k,)).reshape(n, k).copy() if n else np.zeros((0, k), f32)


def _ico_asset(sub):
    p = os.path.join(scenes.asset_dir(), "normal_map_icosphere_%d.obj" % sub)
    v, f = NR.icosphere(sub, 1.0, NR.generic_rotation())
    return scenes.write_obj(p, v.astype(f32), f)


def _dot32(a, b):
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def _planar_uv(s, scale=0.4, axes=(0, 2)):
    """tri_uv of a flattened scene: u, v = 0.5 + scale * two coordinates of each corner"""
    n = s.n_triangles
    out = np.zeros((n, 6), f32)
    for k, ptr in enumerate((s.tri_p0, s.tri_p1, s.tri_p2)):
        p = _arr(ptr, n, 3)
        out[:, 2 * k] = f32(0.5) + f32(scale) * p[:, axes[0]]; out[:, 2 * k + 1] = f32(0.5) + f32(scale) * p[:, axes[1]]
    return out


# ---- 1. the hook -------------------------------------------------------------------------------------------------------------------------------------
def _hook_scene(big):
    """the shape of test_gpu_normals._hook_scene: three small triangles with uvs -- one smooth, one flat, one with mirrored uvs -- a rectangle, a disk and a
    sphere, all with mapped materials; a second rectangle (and, big, the 1280-triangle smooth icosphere) with an unmapped one"""
    rng = np.random.default_rng(21)
    tris = [np.array([(-3.0, -1.0, 0.1), (-1.6, -0.8, -0.2), (-2.4, 0.9, 0.15)]), np.array([(-1.2, -1.0, 0.0), (0.2, -0.9, 0.1), (-0.5, 0.8, -0.1)]),
            np.array([(0.6, -1.0, 0.05), (2.0, -0.7, 0.0), (1.2, 0.9, 0.2)])]
    be = scenes.HostBackend("normal_map_hook")
    be.camera((0, 0, 8), (0, 0, -1), (0, 1, 0), 60.0, 16, 16)
    be.pointlight((0, 0, 6), (10, 10, 10))
    m_tri = be.mat_matte((0.5, 0.5, 0.5)); m_rect = be.mat_matte((0.4, 0.5, 0.6)); m_curved = be.mat_plastic((0.5, 0.3, 0.2), (0.3, 0.3, 0.3), 0.1); m_plain = be.mat_matte((0.7, 0.7, 0.7))
    for k, t in enumerate(tris):
        p = os.path.join(scenes.asset_dir(), "normal_map_hook_tri_%d.obj" % k)
        be.mesh(scenes.write_obj(p, t.astype(f32), np.array([(0, 1, 2)])), False, False, mat=m_tri)
    be.rect(scenes.AXIS_XY, 2.6, 3.8, -0.8, 0.8, 0.1, False, m_rect)
    be.disk((-4.2, 0.0, 0.0), scenes._normalize((0.2, -0.3, 1.0)), 0.7, m_curved)
    be.sphere((5.0, 0.0, 0.0), 0.8, m_curved)
    be.rect(scenes.AXIS_XY, -2.0, 2.0, 1.2 if not big else -2.4, 1.6 if not big else -1.4, 0.0, False, m_plain)
    if big:
        be.mesh(_ico_asset(3), False, False, offset=(0.0, 3.0, 0.0), mat=m_plain)          # 1280 triangles: the 4-wide walk is under the hook
    be.preprocess()
    s = be.flatten().contents
    n = s.n_triangles
    p0, p1, p2, ng = (_arr(x, n, 3) for x in (s.tri_p0, s.tri_p1, s.tri_p2, s.tri_n))
    vn = np.zeros((n, 9), f32); uv = np.zeros((n, 6), f32)
    small = []
    for t in range(n):
        if p0[t, 1] > 1.5:
            for k, p in enumerate((p0, p1, p2)):
                r = p[t].astype(np.float64) - (0.0, 3.0, 0.0)
                vn[t, 3 * k:3 * k + 3] = (r / np.linalg.norm(r)).astype(f32)
        else:
            small.append(t)
    small.sort(key=lambda t: p0[t, 0])
    side = []
    for _ in range(3):                                              # three distinct normals tilted 5 .. 25 degrees
        v = rng.normal(size=3); g = ng[small[0]].astype(np.float64); v -= (v @ g) * g; v /= np.linalg.norm(v)
        a = np.radians(rng.uniform(5, 25)); side.append(np.cos(a) * g + np.sin(a) * v)
    vn[small[0]] = np.concatenate(side).astype(f32)
    for t in small:                                                 # u = 0.5 + 0.12 x, v = 0.5 + 0.4 y, the last triangle with v mirrored
        for k, p in enumerate((p0, p1, p2)):
            uv[t, 2 * k] = f32(0.5) + f32(0.12) * p[t, 0]; uv[t, 2 * k + 1] = f32(0.5) + f32(0.4) * p[t, 1] * (f32(-1) if t == small[2] else f32(1))
    rngm = np.random.default_rng(33)
    maps = []
    for _ in range(2):
        m = rngm.integers(40, 216, (4, 8, 3)).astype(np.uint8); m[..., 2] = rngm.integers(200, 256, (4, 8))
        maps.append(m)
    mats = dict(tri=m_tri, rect=m_rect, curved=m_curved, plain=m_plain)
    mat_map = np.full(s.n_materials, -1, np.int32); strength = np.ones(s.n_materials, f32)
    mat_map[m_tri] = 0; strength[m_tri] = 2.0
    mat_map[m_rect] = 1; strength[m_rect] = 0.5
    mat_map[m_curved] = 0; strength[m_curved] = 1.0
    nm = dict(maps=maps, mat_map=mat_map, strength=strength, tri_uv=uv)
    return be, s, vn, nm, (p0, p1, p2, ng), small, mats


def _set_maps(ctx, nm, s):
    ctx.set_normal_maps(jp.normal_maps(nm["maps"], nm["mat_map"], nm.get("strength"), nm.get("tri_uv"), n_triangles=s.n_triangles))


@pytest.mark.parametrize("big", [False, True])
def test_hook_is_the_host_function(ctx, big):
    be, s, vn, nm, (p0, p1, p2, ng), small, mats = _hook_scene(big)
    ctx.set_vertex_normals(vn)
    _set_maps(ctx, nm, s)
    ctx.upload(be.flatten())
    info = ctx.normal_map_info()
    assert info.n_maps == 2 and info.n_mapped_materials == 3 and info.texel_bytes_device == 2 * 32 * 4 and info.table_bytes_device > 0
    if big:
        assert ctx.build_info().q4_nodes > 0
    rng = np.random.default_rng(5)
    n = 4096
    o = np.stack([rng.uniform(-5, 6, n), rng.uniform(-2.5 if big else -1.5, 4.5 if big else 1.6, n), np.full(n, 6.0)], -1)
    tgt = np.stack([rng.uniform(-5, 6, n), rng.uniform(-2.4 if big else -1.2, 4.2 if big else 1.5, n), np.zeros(n)], -1)
    d = tgt - o; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = o.astype(f32); d = d.astype(f32)
    t0 = np.full(n, 1e-3, f32); t1 = np.full(n, np.inf, f32)
    hit, t, prim_t, nrm_t = ctx.trace(o, d, t0, t1)
    prim, g, ns = ctx.shading_normal(o, d, t0, t1)
    assert np.array_equal(prim, prim_t) and _same(g, nrm_t)
    miss = prim < 0
    assert (g[miss] == 0).all() and (ns[miss] == 0).all()
    pc = np.maximum(prim, 0)
    kind = np.array([s.prim_shape_type[i] for i in range(s.n_primitives)]); idx = np.array([s.prim_shape_index[i] for i in range(s.n_primitives)])
    mat = np.array([s.prim_material[i] for i in range(s.n_primitives)])
    p = (o + t[:, None] * d).astype(f32)                          # ray(distance) as the kernels form it: one fp32 multiply and add per component
    tri = np.where(~miss & (kind[pc] == M.TRIANGLE), idx[pc], -1)
    smooth = (tri >= 0) & vn[np.maximum(tri, 0)].any(-1)
    nb = g.copy()
    k = tri[smooth]
    nb[smooth] = jp.interpolate_normals(p0[k], p1[k], p2[k], ng[k], vn[k], p[smooth])
    # unmapped materials: what they return today
    plain = ~miss & (mat[pc] == mats["plain"])
    assert plain.sum() > 50 and _same(ns[plain], nb[plain]) and (not big or (ns[plain] != g[plain]).any())
    # triangles with the mapped material: bit for bit
    counts = []
    for ti in small:
        sel = tri == ti
        kk = np.full(sel.sum(), ti)
        b0, b1, b2 = NR.barycentrics(p0[kk], p1[kk], p2[kk], p[sel], f32)
        uv6 = nm["tri_uv"][kk]
        uv = np.stack([((b0 * uv6[:, 0]).astype(f32) + (b1 * uv6[:, 2]).astype(f32)).astype(f32) + (b2 * uv6[:, 4]).astype(f32),
                       ((b0 * uv6[:, 1]).astype(f32) + (b1 * uv6[:, 3]).astype(f32)).astype(f32) + (b2 * uv6[:, 5]).astype(f32)], -1).astype(f32)
        du, dv, ok = jp.triangle_tangents(p0[kk], p1[kk], p2[kk], uv6)
        want, on = jp.perturb_normals(nb[sel], g[sel], du, dv, uv, nm["maps"][0], 2.0)
        assert ok.all() and _same(ns[sel], want), "triangle %d" % ti
        counts.append((int(sel.sum()), int(on.sum())))
        assert sel.sum() > 50 and on.mean() > 0.5
    # the mapped rectangle: bit for bit
    rect = ~miss & (kind[pc] == M.RECTANGLE) & (mat[pc] == mats["rect"])
    j = idx[pc][rect]
    r0, r1, r3 = (_arr(x, s.n_rectangles, 3) for x in (s.rect_p0, s.rect_p1, s.rect_p3))
    v01 = (r1[j] - r0[j]).astype(f32); v03 = (r3[j] - r0[j]).astype(f32); v0p = (p[rect] - r0[j]).astype(f32)
    uv = np.stack([(_dot32(v01, v0p) / _dot32(v01, v01)).astype(f32), (_dot32(v03, v0p) / _dot32(v03, v03)).astype(f32)], -1)
    want, on = jp.perturb_normals(nb[rect], g[rect], v01, v03, uv, nm["maps"][1], 0.5)
    assert rect.sum() > 50 and on.mean() > 0.9 and _same(ns[rect], want)
    # sphere and disk: the device's atan2f / asinf may differ from the host's by a few ulp, the lookup is continuous in uv -> the angle bound of the host test
    shapes = M.shapes_of(s)
    worst = 0.0; left_out = 0; total = 0
    for kd in (M.SPHERE, M.DISK):
        sel = ~miss & (kind[pc] == kd)
        i = int(prim[sel][0]); assert (prim[sel] == i).all()
        uv64, du, dv, ok = R.hit_uv_and_tangents(shapes[i], None, p[sel].astype(np.float64))
        ref, ron, margin = R.perturb(g[sel], g[sel], du, dv, uv64, nm["maps"][0], 1.0)
        near = (np.minimum(uv64[:, 0], 1.0 - uv64[:, 0]) < 1e-3) | (uv64[:, 1] < 1e-3) | ((kd == M.SPHERE) & (uv64[:, 1] > 1.0 - 1e-3)) | (margin < 1e-3)
        keep = ~near
        assert sel.sum() > 50 and ron[keep].mean() > 0.9
        got = ns[sel][keep]
        assert np.array_equal((got != g[sel][keep]).any(-1), ron[keep])
        a = R.angle(got[ron[keep]], ref[keep][ron[keep]]).max()
        worst = max(worst, a); left_out += int(near.sum()); total += int(sel.sum())
        counts.append((int(sel.sum()), int(ron.sum())))
    print("hook (%s): %d rays, %d miss; (hits, perturbed) per small triangle, sphere, disk %s; rectangle %d; unmapped %d; sphere / disk: %d of %d left out (near the u seam, a pole, the centre, or within 1e-3 of a decision edge of the definition), largest angle %.3e rad (bound %.3e)" % (
        "big" if big else "tiny", n, miss.sum(), counts, rect.sum(), plain.sum(), left_out, total, worst, ANGLE_BOUND))
    assert left_out <= 0.05 * total
    assert worst <= ANGLE_BOUND
    assert ((ns[~miss] * g[~miss]).sum(-1) > 0).all()


# ---- 2. neutral and absent maps change nothing -------------------------------------------------------------------------------------------------------
def test_neutral_and_absent_maps_change_nothing():
    start = jp.device_bytes_in_use()
    W, H = 64, 48
    be = scenes.build_cornell(scenes.HostBackend("normal_map_noop"), W, H, lambert_only=False)
    s = be.flatten().contents
    rp = jp.render_params(W, H, 4, 5, 99)
    neutral = np.zeros((4, 8, 3), np.uint8); neutral[..., :2] = 128; neutral[..., 2] = 255
    uv = np.random.default_rng(2).uniform(0, 1, (s.n_triangles, 6)).astype(f32)
    fresh = jp.Context(0)                                           # a context that never heard of a map: what every case below must reproduce
    try:
        fresh.upload(be.flatten())
        film0 = fresh.render(rp); g0 = fresh.render_guides(rp, 3)
        assert fresh.normal_map_info().mapped_last_render == 0 and fresh.normal_map_info().n_maps == 0
    finally:
        fresh.close()
    c = jp.Context(0)
    try:
        cases = {"no maps": jp.normal_maps([], np.full(s.n_materials, -1), None, uv),
                 "no material mapped": jp.normal_maps([R.bump_map(16)], np.full(s.n_materials, -1), None, uv),
                 "neutral maps": jp.normal_maps([neutral, neutral[:1, :1]], np.arange(s.n_materials) % 2, np.full(s.n_materials, 3.0, f32), uv),
                 "strength 0": jp.normal_maps([R.bump_map(16)], np.zeros(s.n_materials, np.int32), np.zeros(s.n_materials, f32), uv)}
        for name, m in cases.items():
            c.set_normal_maps(m)
            c.upload(be.flatten())
            film1 = c.render(rp); g1 = c.render_guides(rp, 3)
            i = c.normal_map_info()
            assert i.mapped_last_render == 0 and i.table_bytes_device == 0 and i.texel_bytes_device == 0 and c.normal_info().smooth_last_render == 0, name
            assert _same(film0, film1) and all(_same(a, b) for a, b in zip(g0, g1)), name
        # counts that differ from the scene's are refused at upload, and the context stays usable
        for m, word in ((jp.normal_maps([neutral], np.full(s.n_materials + 1, -1), None, uv), "n_materials"), (jp.normal_maps([neutral], np.full(s.n_materials, -1), None, uv[:-1]), "n_triangles")):
            c.set_normal_maps(m)
            with pytest.raises(jp.JetPbrtError) as e:
                c.upload(be.flatten())
            assert "status %d" % INVALID_ARGUMENT in str(e.value) and word in str(e.value)
        c.set_normal_maps(None)
        c.upload(be.flatten())
        assert _same(c.render(rp), film0)
        # ... and a real map on every material changes the film
        c.set_normal_maps(jp.normal_maps([R.bump_map(16)], np.zeros(s.n_materials, np.int32), None, uv))
        c.upload(be.flatten())
        assert not _same(c.render(rp), film0) and c.normal_map_info().mapped_last_render == 1
    finally:
        c.close()
    assert jp.device_bytes_in_use() == start


# ---- 3. deterministic direct light, per family ---------------------------------------------------------------------------------------------------------
FAMILIES = {"all": dict(mode="all", est="nee", tex=False), "power": dict(mode="power", est="nee", tex=False),
            "mis": dict(mode="power", est="mis", tex=False), "textured": dict(mode="all", est="nee", tex=True)}


def _bump_scene(size=48, tex=False):
    """a 2 x 2 rectangle behind the smooth 80-triangle icosphere (radius 0.5), both matte 0.6 (or a checker of 0.6 / 0.3), seen from (0, -4, 0) along +y,
    one directional light; the bump field on both"""
    be = scenes.HostBackend("normal_map_bump")
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), float(np.degrees(2.0 * np.arctan(TAN_HALF))), size, size)
    wl = np.array([np.sin(np.radians(50.0)), -np.cos(np.radians(50.0)), 0.2]); wl /= np.linalg.norm(wl)
    be.dirlight(tuple(-wl), (3.0, 3.0, 3.0))                       # arriving from wl
    m = be.mat_matte(tex=be.texture_checker((0.6, 0.6, 0.6), (0.3, 0.3, 0.3))) if tex else be.mat_matte((0.6, 0.6, 0.6))
    be.mesh(_ico_asset(1), False, False, scale=0.5, mat=m)
    be.rect(scenes.AXIS_XZ, -1.0, 1.0, -1.0, 1.0, 0.6, False, m)
    be.preprocess()
    s = be.flatten().contents
    nm = dict(maps=[R.bump_map(16)], mat_map=np.zeros(s.n_materials, np.int32), strength=None, tri_uv=_planar_uv(s, 0.9))
    return be, s, NR.radial_normals(s), nm


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_direct_light_of_a_delta_light_equals_the_predictor(ctx, family):
    """Film of the mapped rectangle and smooth icosphere under one directional light, max_depth 1, debug sampler: within 1e-5 absolute of the float64
    predictor on every hit pixel the predictor does not mark fragile (at most 2 % of the hit pixels), and far from the unmapped render."""
    fam = FAMILIES[family]
    be, s, vn, nm = _bump_scene(48, fam["tex"])
    ctx.set_light_sampling(fam["mode"])
    ctx.set_vertex_normals(vn)
    rp = jp.render_params(48, 48, 1, 1, 7, sampler_mode=jp.JP_SAMPLER_DEBUG)
    tex = be.flatten_textures() if fam["tex"] else None
    ctx.upload(be.flatten(), tex)
    ctx.set_estimator(fam["est"])
    plain = ctx.render(rp)
    assert ctx.normal_map_info().mapped_last_render == 0
    _set_maps(ctx, nm, s)
    ctx.upload(be.flatten(), tex)
    film = ctx.render(rp)
    assert ctx.normal_map_info().mapped_last_render == 1 and ctx.normal_info().smooth_last_render == 1
    o, d = NR.camera_rays(s)
    _, _, alb = ctx.surface(o.astype(f32), d.astype(f32), np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32))
    pred, hit, fragile, mapped = R.direct_delta(s, vn, nm, alb)
    flat, _, _, _ = R.direct_delta(s, vn, None, alb)
    keep = hit & ~fragile
    err = np.abs(film.astype(np.float64) - pred).max(-1)
    err_plain = np.abs(plain.astype(np.float64) - flat).max(-1)
    diff = np.abs(film.astype(np.float64) - plain).max(-1)[mapped].mean()
    print("%s: %d hit pixels, %d perturbed, %d fragile; largest error %.3e (kept), %.3e (fragile), unmapped render vs its predictor %.3e; mean |mapped - unmapped| on the mapped pixels %.4f" % (
        family, hit.sum(), mapped.sum(), fragile.sum(), err[keep].max(), err[hit & fragile].max() if (hit & fragile).any() else 0.0, err_plain[keep].max(), diff))
    assert hit.sum() > 700 and mapped.sum() > 0.8 * hit.sum() and fragile.sum() <= 0.02 * hit.sum()
    assert (film[~hit] == 0).all()
    assert err[keep].max() <= 1e-5
    assert diff > 0.01


# ---- 4. the guard ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [False, True])
def test_guard_blacks_a_light_below_the_geometric_plane(ctx, above):
    """one mapped triangle in the plane z = 0 whose one-texel map tilts Ns' 40 degrees toward +x; a point light below the geometric plane but above the
    shading plane gives exactly 0, the light mirrored above the plane gives the predictor's value"""
    be = scenes.HostBackend("normal_map_guard")
    be.camera((0, 0, 4), (0, 0, -1), (0, 1, 0), 30.0, 1, 1)
    lz = 0.3 if above else -0.3
    be.pointlight((3.0, 0.0, lz), (20.0, 20.0, 20.0))
    m = be.mat_matte((0.6, 0.6, 0.6))
    p = os.path.join(scenes.asset_dir(), "normal_map_guard_tri.obj")
    be.mesh(scenes.write_obj(p, np.array([(-2, -2, 0), (2, -2, 0), (0, 3, 0)], f32), np.array([(0, 1, 2)])), False, False, mat=m)
    be.preprocess()
    s = be.flatten().contents
    texel = np.array([[[128 + 107, 128, 255]]], np.uint8)           # atan(107 / 127) = 40.1 degrees toward +u
    uv = np.array([[0.0, 0.0, 1.0, 0.0, 0.5, 1.0]], f32)             # u along +x, v along +y
    assert s.n_triangles == 1 and np.allclose(_arr(s.tri_p0, 1, 3), (-2, -2, 0)) and np.allclose(_arr(s.tri_n, 1, 3), (0, 0, 1))
    ctx.set_normal_maps(jp.normal_maps([texel], [0], None, uv))
    ctx.upload(be.flatten())
    film = ctx.render(jp.render_params(1, 1, 1, 1, 3, sampler_mode=jp.JP_SAMPLER_DEBUG))
    assert ctx.normal_map_info().mapped_last_render == 1
    wi = np.array([3.0, 0.0, lz]); d2 = wi @ wi; wi /= np.sqrt(d2)
    nf = np.array([107.0, 0.0, 127.0]); nf /= np.linalg.norm(nf)
    assert wi @ nf > 0.3 and (wi[2] > 0) == above                   # above the shading plane either way; below the geometric plane unless mirrored
    want = 0.6 / np.pi * (20.0 / d2) * abs(wi @ nf) if above else 0.0
    print("guard (%s the plane): film %r, predicted %.7f" % ("above" if above else "below", film[0, 0].tolist(), want))
    if above:
        assert np.abs(film[0, 0].astype(np.float64) - want).max() <= 1e-5 and want > 0.1
    else:
        assert (film[0, 0] == 0).all()


# ---- 5. the map families -------------------------------------------------------------------------------------------------------------------------------
TINT = (0.05, 0.05, 0.05)                                        # the scene's environment light tints the map: the film stays below the clamp at 1
MAP_SEEDS, MAP_SPP, MAP_SIZE = tuple(range(1000, 1008)), 64, 32  # the seeds, spp and size of test_gpu_normals.test_map_families_match_the_texel_quadrature
_map_ref = {}


def _env_map():
    rgb = np.full((4, 8, 3), 0.05, f32)
    rgb[1, 6] = 40.0                                               # from the camera's side, above the horizon
    return rgb


def _ico_map_scene(tex):
    """the smooth 80-triangle icosphere of test_gpu_normals' map families (convex: what the quadrature of normals_ref.map_direct_rays covers) seen from
    (0, -4, 0), matte 0.6 or a checker of 0.6 / 0.3, lit by the tinted map alone, the bump field on its material"""
    be = scenes.HostBackend("normal_map_env")
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), float(np.degrees(2.0 * np.arctan(TAN_HALF))), MAP_SIZE, MAP_SIZE)
    be.envlight(TINT)
    m = be.mat_matte(tex=be.texture_checker((0.6, 0.6, 0.6), (0.3, 0.3, 0.3))) if tex else be.mat_matte((0.6, 0.6, 0.6))
    be.mesh(_ico_asset(1), False, False, mat=m)
    be.preprocess()
    s = be.flatten().contents
    nm = dict(maps=[R.bump_map(16)], mat_map=np.zeros(s.n_materials, np.int32), strength=None, tri_uv=_planar_uv(s, 0.45))
    return be, s, NR.radial_normals(s), nm


def _map_reference(s, vn, nm):
    """the quadrature at the very camera rays the 8 x 64 samples of a pixel take, computed once for the three families (the geometry, the normals and the
    maps are the same): per ray the hit, the integrals with Ns' and with Ng, the texel a miss sees"""
    if not _map_ref:
        rays = [D.camera_rays(s.camera, MAP_SIZE, MAP_SIZE, seed, k) for seed in MAP_SEEDS for k in range(MAP_SPP)]
        o = np.concatenate([r[0] for r in rays]); d = np.concatenate([r[1] for r in rays])
        _map_ref["rays"] = (o, d)
        _map_ref["ref"] = R.map_direct_rays(s, vn, nm, o, d, _env_map(), TINT, E.UP_Z, through_camera=True)
    return _map_ref["rays"], _map_ref["ref"]


@pytest.mark.parametrize("family", ["map", "map_mis", "map_textured"])
def test_map_families_match_the_texel_quadrature(ctx, family):
    """The mapped smooth icosphere under an 8 x 4 map with one bright texel, POWER_ONE, max_depth 1, 32 x 32: the mean of 8 seeds of 64 spp against the
    float64 quadrature of the direct light over every texel with Ns' in place of Ns; |mean - predicted| <= 5 se + 1e-3 on all but 1 % of the hit pixels,
    and the same quadrature with Ng must fail that on at least 20 % of the lit pixels (the bound of test_gpu_normals' map families)."""
    tex = family == "map_textured"
    be, s, vn, nm = _ico_map_scene(tex)
    ctx.set_environment_map(_env_map(), "z")
    ctx.set_light_sampling("power")
    ctx.set_vertex_normals(vn)
    _set_maps(ctx, nm, s)
    ctx.upload(be.flatten(), be.flatten_textures() if tex else None)
    ctx.set_estimator("mis" if family == "map_mis" else "nee")
    films = np.stack([ctx.render(jp.render_params(MAP_SIZE, MAP_SIZE, MAP_SPP, 1, seed)).astype(np.float64) for seed in MAP_SEEDS])
    assert ctx.normal_map_info().mapped_last_render == 1 and ctx.env_info().mapped_last_render == 1 and ctx.normal_info().smooth_last_render == 1
    (o, d), (hit_r, E_ns, E_ng, miss) = _map_reference(s, vn, nm)
    _, _, alb = ctx.surface(o, d, np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32))
    per_pixel = lambda E_: np.where(hit_r[:, None], alb.astype(np.float64) / np.pi * E_, miss).reshape(len(MAP_SEEDS) * MAP_SPP, MAP_SIZE, MAP_SIZE, 3).mean(0)
    pred, flat = per_pixel(E_ns), per_pixel(E_ng)
    hit = hit_r.reshape(-1, MAP_SIZE, MAP_SIZE).all(0)             # every sample of the pixel hits the mesh (the others: compared all the same, as "not hit")
    mean = films.mean(0); se = films.std(0, ddof=1) / np.sqrt(8.0)
    assert films.max() < 1.0 and pred.max() < 1.0                  # nothing near the film's clamp
    bad = (np.abs(mean - pred) > 5.0 * se + 1e-3).any(-1)
    lit = hit & (pred.max(-1) > 0.01)                              # lit by the bright texel (the rest of the map gives 0.0015 at most)
    bad_flat = (np.abs(mean - flat) > 5.0 * se + 1e-3).any(-1) & lit
    print("%s: %d hit pixels, %d outside 5 se + 1e-3 (largest |mean - predicted| %.3e, largest se %.3e); with Ng in place of Ns' %d of %d lit pixels outside" % (
        family, hit.sum(), bad.sum(), np.abs(mean - pred)[hit].max(), se[hit].max(), bad_flat.sum(), lit.sum()))
    assert hit.sum() > 300 and lit.sum() > 100
    assert bad.sum() <= 0.01 * hit.sum()                           # (silhouette and background pixels included in the count)
    assert bad_flat.sum() >= 0.2 * lit.sum()


# ---- 6. the guides -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True])
def test_normal_guide_is_the_mapped_shading_normal(ctx, lens):
    be, s, vn, nm = _bump_scene(48)
    rp = jp.render_params(48, 48, 1, 1, 11, sampler_mode=jp.JP_SAMPLER_DEBUG)
    if lens:
        ctx.set_lens(0.05, 4.0, 5, 10.0)                            # five blades: the debug sampler's lens point is off the centre
    ctx.set_vertex_normals(vn)
    ctx.upload(be.flatten())
    plain = ctx.render_guides(rp, 1)
    _set_maps(ctx, nm, s)
    ctx.upload(be.flatten())
    alb, nrm, dep = ctx.render_guides(rp, 1)
    y, x = np.mgrid[0:48, 0:48]
    o, d, _ = ctx.camera_rays(rp, x.ravel(), y.ravel(), np.zeros(48 * 48, np.int32))
    if lens:
        assert (o != o[0]).any() or (o[0] != np.array([0, -4, 0], f32)).any()
    prim, g, ns = ctx.shading_normal(o, d, np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32))
    assert _same(nrm, ns.reshape(48, 48, 3))
    assert _same(alb, plain[0]) and _same(dep, plain[2])           # albedo and depth are the unmapped scene's
    hitm = dep > 0
    assert hitm.sum() > 700 and (nrm[hitm] != plain[1][hitm]).any(-1).mean() > 0.9


# ---- 8. refusals and fallbacks --------------------------------------------------------------------------------------------------------------------------------
def test_whitted_refuses_fused_falls_back_debug_ignores_and_profiling_times(ctx):
    be, s, vn, nm = _bump_scene(32)
    ctx.upload(be.flatten())
    dbg0 = ctx.render(jp.render_params(32, 32, 1, 3, 5, integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))
    _set_maps(ctx, nm, s)
    ctx.set_options(fused=1)
    ctx.upload(be.flatten())
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.render(jp.render_params(32, 32, 1, 3, 5, integrator=jp.JP_INTEGRATOR_WHITTED))
    assert "status %d" % UNSUPPORTED in str(e.value) and "normal maps" in str(e.value)
    dbg = ctx.render(jp.render_params(32, 32, 1, 3, 5, integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))     # ignores the maps
    assert ctx.normal_map_info().mapped_last_render == 0 and _same(dbg, dbg0)
    ctx.set_profiling(True)
    film = ctx.render(jp.render_params(32, 32, 2, 3, 5))
    i = ctx.normal_map_info()
    cnt = ctx.counters()
    print("profiling: normal_map_ms %.4f of shade_ms %.4f" % (i.normal_map_ms, cnt.shade_ms))
    assert i.mapped_last_render == 1 and film.mean() > 0.005 and np.isfinite(film).all()
    assert ctx.build_info().fused_last_render == 0
    assert 0 < i.normal_map_ms < cnt.shade_ms
    # a refusal of jp_set_normal_maps leaves the state alone
    with pytest.raises(jp.JetPbrtError):
        ctx.set_normal_maps(jp.normal_maps(nm["maps"], nm["mat_map"], np.full(s.n_materials, np.nan, f32), nm["tri_uv"]))
    ctx.upload(be.flatten())
    assert ctx.normal_map_info().n_mapped_materials == s.n_materials


# ---- 7. host API ----------------------------------------------------------------------------------------------------------------------------------------------
def test_host_render_equals_the_c_abi_render(ctx):
    """FMaterial::normalMap through the host library (a map from memory on the mesh, whose OBJ carries vt, and a FromHeight map on the rectangle) renders the
    film of the C ABI path bit for bit"""
    v, f = NR.icosphere(1, 1.0, NR.generic_rotation())
    path = scenes.write_obj(os.path.join(scenes.asset_dir(), "normal_map_ico_vt.obj"), v.astype(f32), f, uvs=(0.5 + 0.45 * v[:, [0, 2]]).astype(f32))
    height = (127.5 + 127.5 * np.sin(np.arange(16) * 0.8)[None, :] * np.cos(np.arange(16) * 0.5)[:, None]).astype(np.uint8)

    def build(mapped):
        be = scenes.HostBackend("normal_map_host_api")
        be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), 40.0, 32, 32)
        be.pointlight((3.0, -3.0, 2.0), (30.0, 30.0, 30.0))
        a = be.mat_plastic((0.5, 0.3, 0.2), (0.3, 0.3, 0.3), 0.1); b = be.mat_matte((0.6, 0.6, 0.6))
        if mapped:
            be.mat_set_normal_map(a, be.normal_map(R.bump_map(16)), 1.5)
            be.mat_set_normal_map(b, be.normal_map_from_height(height, 4.0))
        be.mesh(path, False, False, scale=0.6, mat=a)
        be.rect(scenes.AXIS_XZ, -1.2, 1.2, -1.2, 1.2, 0.8, False, b)
        be.preprocess()
        return be
    be = build(True)
    film = np.zeros((32, 32, 3), f32)
    cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, 32, 32, 4, 3, 77, 0, 0, 1, film.ctypes.data, cnt) == 0
    nm = be.flatten_normal_maps()
    assert nm is not None and nm.n_maps == 2 and nm.n_triangles == 80 and jp.check_normal_maps(nm) == 2
    ctx.set_normal_maps(nm)
    ctx.upload(be.flatten())
    got = ctx.render(jp.render_params(32, 32, 4, 3, 77))
    assert ctx.normal_map_info().mapped_last_render == 1 and ctx.normal_map_info().n_mapped_materials == 2
    assert _same(film, got) and film.mean() > 0.01
    plain = build(False)
    assert plain.flatten_normal_maps() is None
    film_plain = np.zeros((32, 32, 3), f32)
    assert jp.host_lib().jp_host_render(plain.h, 32, 32, 4, 3, 77, 0, 0, 1, film_plain.ctypes.data, cnt) == 0
    assert not _same(film, film_plain)
