"""INTEGRATION.md "Vertex normals" restated in numpy -- the interpolated shading normal operation by operation in float32 (the bit-exact yardstick) and in
float64, the computed-normal rule of the host API (angle-weighted, crease angle A), the icosphere the tests render, and float64 predictors of the direct
light on a mesh with vertex normals: per pixel-centre ray the closest hit, Ns, the hemisphere test in the Ns frame, the guard on Ng and occlusion, for a
delta light and (by quadrature over the texels) for an environment map.  Written from the definition text, not from the C++; the scene reader and the ray
caster are those of tests/mis_ref.py."""
import numpy as np

import envmap_ref as E
import mis_ref as M

f32 = np.float32


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def barycentrics(p0, p1, p2, p, dt):
    """b0, b1, b2 by the normal equations in dtype dt, every operation rounded to dt in the order written; b1 = b2 = 0 when den == 0"""
    p0, p1, p2, p = (np.asarray(x, dt) for x in (p0, p1, p2, p))
    e, f, g = p1 - p0, p2 - p0, p - p0
    d00, d01, d11, d20, d21 = _dot32(e, e), _dot32(e, f), _dot32(f, f), _dot32(g, e), _dot32(g, f)
    den = d00 * d11 - d01 * d01
    with np.errstate(divide="ignore", invalid="ignore"):
        b1 = np.where(den != 0, (d11 * d20 - d01 * d21) / den, dt(0))
        b2 = np.where(den != 0, (d00 * d21 - d01 * d20) / den, dt(0))
    b0 = dt(1) - b1 - b2
    return b0.astype(dt), b1.astype(dt), b2.astype(dt)


def _interpolate(p0, p1, p2, ng, vn9, p, dt):
    ng = np.asarray(ng, dt); vn9 = np.asarray(vn9, dt).reshape(-1, 9)
    b0, b1, b2 = barycentrics(p0, p1, p2, p, dt)
    n0, n1, n2 = vn9[:, 0:3], vn9[:, 3:6], vn9[:, 6:9]
    m = (b0[:, None] * n0 + b1[:, None] * n1) + b2[:, None] * n2
    l2 = _dot32(m, m)
    ok = (l2 > 0) & np.isfinite(l2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ns = m / np.sqrt(np.where(ok, l2, dt(1)))[:, None]
    ns = np.where((_dot32(ns, ng) < 0)[:, None], -ns, ns)
    return np.where(ok[:, None], ns, ng).astype(dt)


def interpolate32(p0, p1, p2, ng, vn9, p):
    """Ns for n points: (n, 3) arrays, vn9 (n, 9) -> (n, 3) float32, bit for bit what the definition gives in fp32"""
    return _interpolate(p0, p1, p2, ng, vn9, p, np.float32)


def interpolate64(p0, p1, p2, ng, vn9, p):
    return _interpolate(p0, p1, p2, ng, vn9, p, np.float64)


# ---- computed normals (FScene::CreateTriangleMesh(..., angle A)) ----------------------------------------------------------------------------------------
def computed_normals(verts, faces, angle_deg):
    """corner k of triangle T at position index v gets normalize(sum of angle_U(v) * Ng_U over the triangles U sharing v with dot(Ng_T, Ng_U) >= cos A);
    T itself always; float64, face order; a zero sum gives Ng_T.  -> (n_faces, 3, 3)"""
    verts = np.asarray(verts, np.float64); faces = np.asarray(faces)
    cosA = np.cos(np.radians(angle_deg))
    ng = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    ng = ng / np.linalg.norm(ng, axis=-1, keepdims=True)
    ang = np.zeros((len(faces), 3))
    for k in range(3):
        a = verts[faces[:, (k + 1) % 3]] - verts[faces[:, k]]; b = verts[faces[:, (k + 2) % 3]] - verts[faces[:, k]]
        c = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
        ang[:, k] = np.arccos(np.clip(c, -1.0, 1.0))
    users = {}
    for t, f in enumerate(faces):
        for k in range(3):
            users.setdefault(int(f[k]), []).append((t, k))
    out = np.zeros((len(faces), 3, 3))
    for t, f in enumerate(faces):
        for k in range(3):
            s = np.zeros(3)
            for (u, ku) in users[int(f[k])]:
                if u == t or ng[t] @ ng[u] >= cosA:
                    s = s + ang[u, ku] * ng[u]
            l = np.linalg.norm(s)
            out[t, k] = s / l if l > 0 else ng[t]
    return out


# ---- meshes of the tests ------------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=1, radius=1.0, rotation=None):
    """unit icosahedron subdivided `subdivisions` times (20 * 4^k triangles), vertices pushed onto the sphere, outward winding -> (verts float64, faces)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]; v.append(x / np.linalg.norm(x)); mid[k] = len(v) - 1
            return mid[k]
        for (a, b, c) in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v) * radius
    if rotation is not None:
        v = v @ np.asarray(rotation, np.float64).T
    return v, np.array(f)


def generic_rotation():
    """a rotation with no symmetry axis of the icosahedron along a coordinate axis"""
    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        r = np.eye(3); i, j = [(1, 2), (2, 0), (0, 1)][axis]
        r[i, i] = c; r[i, j] = -s; r[j, i] = s; r[j, j] = c
        return r
    return rot(2, 0.7) @ rot(1, 0.4) @ rot(0, 1.1)


def radial_normals(s, center=(0.0, 0.0, 0.0)):
    """tri_vn of a flattened scene whose triangles lie on a sphere about `center`: the normalised vertex positions, (n_triangles, 9) float32"""
    n = s.n_triangles
    out = np.zeros((n, 9), np.float32)
    for k, ptr in enumerate((s.tri_p0, s.tri_p1, s.tri_p2)):
        p = np.array([ptr[i] for i in range(3 * n)], np.float64).reshape(n, 3) - np.asarray(center, np.float64)
        out[:, 3 * k:3 * k + 3] = (p / np.linalg.norm(p, axis=-1, keepdims=True)).astype(np.float32)
    return out


def prim_normals(s, tri_vn):
    """per primitive of the flattened scene: its nine normals or None (flat triangle, other shape)"""
    tri_vn = np.asarray(tri_vn, np.float64).reshape(-1, 9)
    out = []
    for i in range(s.n_primitives):
        v = tri_vn[s.prim_shape_index[i]] if s.prim_shape_type[i] == M.TRIANGLE else None
        out.append(v if v is not None and v.any() else None)
    return out


# ---- the camera and the first hit ------------------------------------------------------------------------------------------------------------------
def camera_rays(s):
    """pixel-centre rays of the flattened scene's camera (JP_SAMPLER_DEBUG), row-major top row first -> (o (n, 3), d (n, 3)) float64"""
    c = s.camera
    W, H = int(c.res_x), int(c.res_y)
    pos, front, right, up = (np.array(list(x), np.float64) for x in (c.pos, c.front, c.right, c.up))
    y, x = np.mgrid[0:H, 0:W]
    fx, fy = x.ravel() + 0.5, y.ravel() + 0.5
    d = front + right * (fx / W - 0.5)[:, None] + up * (0.5 - fy / H)[:, None]
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(pos, d.shape).copy(), d


def _silhouette_edges(shapes, eye):
    """per triangle, per edge (opposite p0, p1, p2): the triangle across it faces the other way from `eye`, or there is none"""
    key = lambda p: tuple(np.round(p, 6))
    facing = [None if sh["kind"] != M.TRIANGLE else bool(sh["n"] @ (eye - sh["p0"]) > 0) for sh in shapes]
    edges = {}
    for i, sh in enumerate(shapes):
        if sh["kind"] != M.TRIANGLE:
            continue
        ps = [sh["p0"], sh["p1"], sh["p2"]]
        for e in range(3):
            a, b = key(ps[(e + 1) % 3]), key(ps[(e + 2) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((i, e))
    sil = {i: [True, True, True] for i, sh in enumerate(shapes) if sh["kind"] == M.TRIANGLE}
    for users in edges.values():
        if len(users) == 2:
            (i, e), (j, g) = users
            same = facing[i] == facing[j]
            sil[i][e] = not same; sil[j][g] = not same
    return sil


def _camera_intersect(s, shapes, o, d):
    """M.intersect for rays through the scene's camera in row-major pixel order, one block of pixels after another (the samples of a frame): a triangle
    is tested against the rays of the pixels its projection's bounding box touches (one pixel of margin), anything else against all of them"""
    c = s.camera
    W, H = int(c.res_x), int(c.res_y)
    pos, front, right, up = (np.array(list(x), np.float64) for x in (c.pos, c.front, c.right, c.up))
    n = len(o)
    best = np.full(n, np.inf); prim = np.full(n, -1)
    pix = np.arange(n) % (W * H)
    px, py = pix % W, pix // W
    for i, sh in enumerate(shapes):
        sel = None
        if sh["kind"] == M.TRIANGLE:
            v = np.array([sh["p0"], sh["p1"], sh["p2"]]) - pos
            z = v @ front
            if (z > 1e-6).all():
                x = ((v @ right) / ((right @ right) * z) + 0.5) * W; y = (0.5 - (v @ up) / ((up @ up) * z)) * H
                sel = np.where((px >= np.floor(x.min()) - 1) & (px <= np.floor(x.max()) + 1) & (py >= np.floor(y.min()) - 1) & (py <= np.floor(y.max()) + 1))[0]
        if sel is None:
            sel = np.arange(n)
        if len(sel) == 0:
            continue
        p1, t1, _, _ = M.intersect([sh], o[sel], d[sel])
        take = (p1 >= 0) & (t1 < best[sel])
        best[sel[take]] = t1[take]; prim[sel[take]] = i
    return prim, best


def first_hits(s, tri_vn, o, d, through_camera=False):
    """closest hits of rays with the scene -> dict(prim, t, p, ng (the normal k_shade uses: rectangles face the ray), ns, smooth, edge (distance in
    barycentrics to the nearest silhouette edge, inf for other shapes)).  through_camera: the rays are samples of the scene's camera, frame after frame"""
    shapes = M.shapes_of(s)
    pn = prim_normals(s, tri_vn)
    if through_camera:
        prim, t = _camera_intersect(s, shapes, o, d)
    else:
        prim, t, _, _ = M.intersect(shapes, o, d)
    n = len(prim)
    p = o + np.where(prim >= 0, t, 0.0)[:, None] * d
    ng = np.zeros((n, 3)); ns = np.zeros((n, 3)); smooth = np.zeros(n, bool); edge = np.full(n, np.inf)
    sil = _silhouette_edges(shapes, o[0])
    for i, sh in enumerate(shapes):
        m = prim == i
        if not m.any():
            continue
        if sh["kind"] == M.SPHERE:
            g = (p[m] - sh["c"]) / np.linalg.norm(p[m] - sh["c"], axis=-1, keepdims=True)
        elif sh["kind"] == M.RECTANGLE:
            g = np.where(((d[m] @ sh["n"]) <= 0)[:, None], sh["n"], -sh["n"])
        else:
            g = np.broadcast_to(sh["n"], (int(m.sum()), 3))
        ng[m] = g; ns[m] = g
        if sh["kind"] == M.TRIANGLE:
            k = int(m.sum())
            rep = lambda x: np.broadcast_to(x, (k, len(x)))
            b = np.stack(barycentrics(rep(sh["p0"]), rep(sh["p1"]), rep(sh["p2"]), p[m], np.float64), -1)
            e = np.where(np.array(sil[i])[None, :], np.abs(b), np.inf).min(-1)
            edge[m] = e
            if pn[i] is not None:
                ns[m] = interpolate64(rep(sh["p0"]), rep(sh["p1"]), rep(sh["p2"]), rep(sh["n"]), rep(pn[i]), p[m])
                smooth[m] = True
    return dict(prim=prim, t=t, p=p, ng=ng, ns=ns, smooth=smooth, edge=edge, shapes=shapes)


# ---- direct light of a delta light on Lambert surfaces (max_depth 1, pixel-centre rays: the film depends on no draw) ------------------------------------
def direct_delta(s, tri_vn, albedo, use_ng=False):
    """the film of a scene of matte surfaces lit by its one directional light, (H, W, 3) float64, with (hit, fragile, lit_by_ns_only, lit_by_ng_only) masks
    (H, W).  albedo: (n_pixels, 3), the colour of the hit (jp_surface's).  use_ng: shade with Ng in place of Ns (what a flat render gives)."""
    W, H = int(s.camera.res_x), int(s.camera.res_y)
    assert s.n_lights == 1 and s.light_type[0] == M.L_DIR
    wi = -np.array([s.light_vec[k] for k in range(3)], np.float64)
    Li = np.array([s.light_radiance[k] for k in range(3)], np.float64)
    o, d = camera_rays(s)
    h = first_hits(s, tri_vn, o, d)
    hit = h["prim"] >= 0
    N = h["ng"] if use_ng else h["ns"]
    wo = -d
    a_wo, a_wi = (wo * N).sum(-1), N @ wi
    g_wo, g_wi = (wo * h["ng"]).sum(-1), h["ng"] @ wi
    hemi = a_wo * a_wi > 0
    guard = np.where(h["smooth"] & (not use_ng), g_wo * g_wi > 0, True)
    # occlusion: a shadow ray from the hit toward the light
    op, _, _, _ = M.intersect(h["shapes"], h["p"], np.broadcast_to(wi, h["p"].shape))
    vis = op < 0
    lit = hit & hemi & guard & vis
    L = np.where(lit[:, None], np.asarray(albedo, np.float64) / np.pi * Li * np.abs(a_wi)[:, None], 0.0)
    signs = np.stack([a_wo, a_wi, g_wo, g_wi, g_wo * g_wi, a_wo * a_wi], -1)
    fragile = hit & ((np.abs(signs) < 1e-4).any(-1) | (h["edge"] < 1e-4))
    n_only = hit & hemi & vis & ~guard                   # lit by Ns, blacked by the guard
    hemi_g = g_wo * g_wi > 0
    g_only = hit & hemi_g & vis & ~hemi                   # the other way round: lit by Ng, dark in the Ns frame
    shp = (H, W)
    return np.clip(L, 0.0, 1.0).reshape(H, W, 3), hit.reshape(shp), fragile.reshape(shp), n_only.reshape(shp), g_only.reshape(shp)


# ---- direct light of an environment map on a convex Lambert mesh (quadrature over the texels) -------------------------------------------------------------
def _map_quadrature(rgb, up, sub_dim, sub_bright):
    """midpoints of sub x sub cells, uniform in (cos theta, phi), of every texel (sub_bright for the texels above ten times the map's median, whose share
    of the film the visibility and guard boundaries cut with an error of the order 1 / sub) -> (world directions (Q, 3), radiance * solid angle (Q, 3))"""
    Hm, Wm = rgb.shape[:2]
    bright = 10.0 * np.median(rgb.sum(-1))
    ws, ls = [], []
    for r in range(Hm):
        c0, c1 = np.cos(np.pi * r / Hm), np.cos(np.pi * (r + 1) / Hm)
        for c in range(Wm):
            if not rgb[r, c].any():
                continue
            sub = sub_bright if rgb[r, c].sum() > bright else sub_dim
            u = (np.arange(sub) + 0.5) / sub
            ct = c0 + (c1 - c0) * u
            st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
            ph = 2.0 * np.pi * (c + u) / Wm
            wm = np.stack([np.outer(st, np.cos(ph)), np.outer(st, np.sin(ph)), np.outer(ct, np.ones(sub))], -1).reshape(-1, 3)   # map space, z up
            ws.append(wm if up == E.UP_Z else wm[:, [1, 2, 0]])                 # JP_ENV_UP_Y: map (x, y, z) = world (z, x, y)
            ls.append(np.broadcast_to(rgb[r, c] * ((c0 - c1) * (2.0 * np.pi / Wm) / (sub * sub)), (sub * sub, 3)))
    return np.concatenate(ws), np.concatenate(ls)


def map_direct_rays(s, tri_vn, o, d, rgb, tint, up, sub_dim=3, sub_bright=24, through_camera=False):
    """Rays (o, d) against a convex mesh under a lat-long map (tinted): per ray the hit, and the integral over the map of radiance * |dot(w, N)| over the
    directions that pass the hemisphere test in the N frame, the guard on Ng (smooth triangles, N = Ns) and, the mesh being convex, dot(Ng, w) > 0 as the
    only visibility term -- once with N = Ns and once with N = Ng (what a flat render integrates).  A miss sees the texel of its direction.
    -> (hit (n,), E_ns (n, 3), E_ng (n, 3), texel radiance of the direction (n, 3)); the direct light of a matte hit is albedo / pi * E."""
    rgb = np.asarray(rgb, np.float64) * np.asarray(tint, np.float64)
    Hm, Wm = rgb.shape[:2]
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    h = first_hits(s, tri_vn, o, d, through_camera)
    hit = h["prim"] >= 0
    W, LdW = _map_quadrature(rgb, up, sub_dim, sub_bright)
    E_ns = np.zeros((len(d), 3)); E_ng = np.zeros((len(d), 3))
    wo = -d
    for i in np.unique(h["prim"][hit]):
        m = np.where(h["prim"] == i)[0]
        for lo in range(0, len(m), 16384):
            k = m[lo:lo + 16384]
            ng = h["ng"][k]
            g_wi = ng @ W.T                                                   # (the facet's normal: the same row for every ray, kept general)
            g_wo = (wo[k] * ng).sum(-1)[:, None]
            vis = g_wi > 0
            for N, out, guard in ((h["ns"][k], E_ns, h["smooth"][k][:, None]), (ng, E_ng, np.zeros((len(k), 1), bool))):
                a_wi = N @ W.T
                a_wo = (wo[k] * N).sum(-1)[:, None]
                ok = vis & (a_wo * a_wi > 0) & np.where(guard, g_wo * g_wi > 0, True)
                out[k] = np.where(ok, np.abs(a_wi), 0.0) @ LdW
    idx, _ = E.lookup(d, Wm, Hm, up)
    return hit, E_ns, E_ng, rgb.reshape(-1, 3)[idx]


def direct_map(s, tri_vn, albedo, rgb, tint, up, use_ng=False, sub_dim=16, sub_bright=160):
    """the expected film at max_depth 1 of a convex matte mesh under a lat-long map through the pixel-centre rays, (H, W, 3) float64 not clamped, and
    the hit mask"""
    W, H = int(s.camera.res_x), int(s.camera.res_y)
    o, d = camera_rays(s)
    hit, E_ns, E_ng, miss = map_direct_rays(s, tri_vn, o, d, rgb, tint, up, sub_dim, sub_bright)
    L = np.where(hit[:, None], np.asarray(albedo, np.float64) / np.pi * (E_ng if use_ng else E_ns), miss)
    return L.reshape(H, W, 3), hit.reshape(H, W)
