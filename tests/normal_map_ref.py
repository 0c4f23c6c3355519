"""Float64 restatement of the normal-map definition (INTEGRATION.md "Normal maps"), written from the definition, not from include/jp_normal_map.h:
the decode, the bilinear lookup with clamp addressing, the tangent frame, the perturbed normal with its "unperturbed" cases and the margins by which
each decision was taken, the triangle tangents, and the uv functions of sphere and disk with their dpdu / dpdv."""
import numpy as np

f64 = np.float64


def decode(b):
    """a byte -> a tangent-space component: 128 -> 0, 255 -> 1, never below -1"""
    return np.maximum((np.asarray(b, f64) - 128.0) / 127.0, -1.0)


def lookup(rgb8, u, v):
    """bilinear between texel centres, clamp addressing; rgb8 (H, W, 3) uint8, top row first; u, v (n,) -> (n, 3)"""
    H, W = rgb8.shape[:2]
    m = decode(rgb8)
    u = np.asarray(u, f64); v = np.asarray(v, f64)
    u = np.where(np.isnan(u), 0.0, np.clip(u, 0.0, 1.0)); v = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 1.0))
    x = u * W - 0.5; y = (1.0 - v) * H - 0.5
    x0 = np.floor(x); y0 = np.floor(y); fx = (x - x0)[:, None]; fy = (y - y0)[:, None]
    i0 = np.clip(x0.astype(int), 0, W - 1); i1 = np.clip(x0.astype(int) + 1, 0, W - 1)
    j0 = np.clip(y0.astype(int), 0, H - 1); j1 = np.clip(y0.astype(int) + 1, 0, H - 1)
    r0 = m[j0, i0] + fx * (m[j0, i1] - m[j0, i0])
    r1 = m[j1, i0] + fx * (m[j1, i1] - m[j1, i0])
    return r0 + fy * (r1 - r0)


def _dot(a, b):
    return (a * b).sum(-1)


def perturb(nb, ng, dpdu, dpdv, uv, rgb8, strength):
    """-> ns (n, 3) (nb where unperturbed), perturbed (n,) bool, margin (n,): how far the closest of the decisions (|mx| + |my| != 0, |T|^2 > 0 relative
    to |dpdu|^2, dot(Ns', N) > 0) was from its edge; a point whose margin is small may legitimately be decided the other way in fp32"""
    nb, ng, dpdu, dpdv, uv = (np.asarray(a, f64) for a in (nb, ng, dpdu, dpdv, uv))
    m = lookup(rgb8, uv[:, 0], uv[:, 1])
    mx = m[:, 0] * strength; my = m[:, 1] * strength; mz = m[:, 2]
    with np.errstate(all="ignore"):
        T = dpdu - nb * _dot(nb, dpdu)[:, None]
        t2 = _dot(T, T)
        okT = np.isfinite(t2) & (t2 > 0)
        T = T / np.sqrt(np.where(okT, t2, 1.0))[:, None]
        B = dpdv - nb * _dot(nb, dpdv)[:, None]
        B = B - T * _dot(T, B)[:, None]
        b2 = _dot(B, B)
        okB = np.isfinite(b2) & (b2 > 0)
        B = np.where(okB[:, None], B / np.sqrt(np.where(okB, b2, 1.0))[:, None], np.cross(nb, T))
        n = (mx[:, None] * T + my[:, None] * B) + mz[:, None] * nb
        n2 = _dot(n, n)
        okN = np.isfinite(n2) & (n2 > 0)
        ns = n / np.sqrt(np.where(okN, n2, 1.0))[:, None]
        side = _dot(ns, ng)
        on = ~((mx == 0) & (my == 0)) & okT & okN & (side > 0)
        rel_t = np.where(_dot(dpdu, dpdu) > 0, t2 / np.where(_dot(dpdu, dpdu) > 0, _dot(dpdu, dpdu), 1.0), 0.0)
        margin = np.minimum(np.minimum(np.abs(mx) + np.abs(my), np.abs(side)), np.minimum(rel_t, np.where(okN, n2, 0.0)))
    return np.where(on[:, None], ns, nb), on, margin


def triangle_tangents(p0, p1, p2, uv6):
    """-> dpdu, dpdv (n, 3), ok (n,) bool"""
    p0, p1, p2, uv6 = (np.asarray(a, f64) for a in (p0, p1, p2, uv6))
    e1 = p1 - p0; e2 = p2 - p0
    du1 = uv6[:, 2] - uv6[:, 0]; dv1 = uv6[:, 3] - uv6[:, 1]; du2 = uv6[:, 4] - uv6[:, 0]; dv2 = uv6[:, 5] - uv6[:, 1]
    det = du1 * dv2 - dv1 * du2
    ok = np.isfinite(det) & (det != 0)
    s = np.where(det > 0, 1.0, -1.0)[:, None]
    dpdu = s * (dv2[:, None] * e1 - dv1[:, None] * e2)
    dpdv = s * (du1[:, None] * e2 - du2[:, None] * e1)
    return np.where(ok[:, None], dpdu, 0.0), np.where(ok[:, None], dpdv, 0.0), ok


# ---- sphere and disk: the uv of GetUV and the directions of increasing u and v ------------------------------------------------------------------------
def sphere_uv(d):
    """d = (p - centre) / radius (unit up to the rounding of p; not normalised again) -> (u, v): phi = atan2(d.z, d.x), theta = asin(d.y), u = 1 - (phi + pi) / 2pi, v = (theta + pi/2) / pi"""
    d = np.asarray(d, f64)
    phi = np.arctan2(d[:, 2], d[:, 0]); theta = np.arcsin(np.clip(d[:, 1], -1.0, 1.0))
    return np.stack([1.0 - (phi + np.pi) / (2 * np.pi), (theta + np.pi / 2) / np.pi], -1)


def sphere_tangents(d):
    d = np.asarray(d, f64)
    dpdu = np.stack([d[:, 2], np.zeros(len(d)), -d[:, 0]], -1)
    dpdv = np.stack([-d[:, 0] * d[:, 1], d[:, 0] ** 2 + d[:, 2] ** 2, -d[:, 1] * d[:, 2]], -1)
    return dpdu, dpdv


def frame(normal):
    """FFrame(normal): n = normalize(normal), t = normalize(cross(n, |n.x| > 0.99 ? (0,1,0) : (1,0,0))), s = normalize(cross(t, n))"""
    n = np.asarray(normal, f64); n = n / np.linalg.norm(n)
    tmp = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.99 else np.array([1.0, 0.0, 0.0])
    t = np.cross(n, tmp); t /= np.linalg.norm(t)
    s = np.cross(t, n); s /= np.linalg.norm(s)
    return s, t, n


def disk_uv(normal, radius, v0):
    """v0 = p - centre -> (u, v): l = (dot(s, v0), dot(t, v0)), phi = atan2(l.y, l.x) wrapped to [0, 2pi), u = phi / 2pi, v = |v0| / radius"""
    s, t, _ = frame(normal)
    v0 = np.asarray(v0, f64)
    phi = np.arctan2(v0 @ t, v0 @ s); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    return np.stack([phi / (2 * np.pi), np.linalg.norm(v0, axis=-1) / radius], -1)


def disk_tangents(normal, v0):
    s, t, _ = frame(normal)
    v0 = np.asarray(v0, f64)
    lx = v0 @ s; ly = v0 @ t
    return t[None] * lx[:, None] - s[None] * ly[:, None], v0.copy()


def angle(a, b):
    """the angle between unit vectors, accurate near 0"""
    a = np.asarray(a, f64); b = np.asarray(b, f64)
    return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.linalg.norm(a / np.linalg.norm(a, axis=-1, keepdims=True) - b / np.linalg.norm(b, axis=-1, keepdims=True), axis=-1)))


def bump_map(size=16, amp=0.6):
    """a smooth bump field as an RGB8 normal map: the normals of the height field amp * sin(2 pi x) * sin(2 pi y) / (2 pi) over the unit square, x right, y up"""
    c = (np.arange(size) + 0.5) / size
    x, y_up = np.meshgrid(c, 1.0 - c)                                # row 0 is the top row: v = 1
    n = np.stack([-amp * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y_up), -amp * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y_up), np.ones_like(x)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return np.clip(np.rint(n * 127.0 + 128.0), 0, 255).astype(np.uint8)


# ---- the mapped Ns of first hits, and the direct light of a directional light on matte surfaces (the pattern of normals_ref.direct_delta) ---------------
def hit_uv_and_tangents(sh, tri_uv6, p):
    """float64 uv, dpdu, dpdv, ok at the points p (k, 3) of one shape dict of mis_ref.shapes_of; tri_uv6: the triangle's six uv values or None"""
    import mis_ref as M
    import normals_ref as NR
    k = len(p)
    rep = lambda x: np.broadcast_to(np.asarray(x, f64), (k, len(x)))
    ok = np.ones(k, bool)
    if sh["kind"] == M.TRIANGLE:
        if tri_uv6 is None:
            return np.zeros((k, 2)), np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k, bool)
        b0, b1, b2 = NR.barycentrics(rep(sh["p0"]), rep(sh["p1"]), rep(sh["p2"]), p, f64)
        t =np.asarray(tri_uv6, f64).reshape(3, 2)
        uv = b0[:, None] * t[0] + b1[:, None] * t[1] + b2[:, None] * t[2]
        du, dv, ok1 = triangle_tangents(sh["p0"][None], sh["p1"][None], sh["p2"][None], np.asarray(tri_uv6, f64)[None])
        return uv, rep(du[0]), rep(dv[0]), ok & ok1[0]
    if sh["kind"] == M.RECTANGLE:
        a = sh["p1"] - sh["p0"]; b = sh["p3"] - sh["p0"]; q = p - sh["p0"]
        return np.stack([q @ a / (a @ a), q @ b / (b @ b)], -1), rep(a), rep(b), ok
    if sh["kind"] == M.SPHERE:
        d = (p - sh["c"]) / sh["r"]
        du, dv = sphere_tangents(d)
        return sphere_uv(d), du, dv, ok                              # GetUV takes (p - centre) / radius as it is: |d| = 1 only up to the rounding of p
    v0 = p - sh["c"]
    du, dv = disk_tangents(sh["n"], v0)
    return disk_uv(sh["n"], sh["r"], v0), du, dv, ok


def mapped_hits(s, tri_vn, nm, o, d, through_camera=False, first_hits=None):
    """normals_ref.first_hits with the maps on top: nm = dict(maps=[(H, W, 3) uint8], mat_map, strength (or None), tri_uv (n_triangles, 6) or None).
    Adds uv, perturbed (bool), margin (of the map's decisions; inf where no map applies) and replaces ns; `record`: the side record is on (guard applies).
    through_camera: as normals_ref.first_hits takes it; first_hits: the function to build on (default normals_ref.first_hits)"""
    import mis_ref as M
    import normals_ref as NR
    h = (first_hits or NR.first_hits)(s, tri_vn if tri_vn is not None else np.zeros((max(1, s.n_triangles), 9)), o, d, through_camera)
    n = len(h["prim"])
    h["uv"] = np.zeros((n, 2)); h["perturbed"] = np.zeros(n, bool); h["margin"] = np.full(n, np.inf); h["nb"] = h["ns"].copy()
    for i, sh in enumerate(h["shapes"]):
        m = h["prim"] == i
        mat = s.prim_material[i]
        if not m.any() or mat < 0 or nm["mat_map"][mat] < 0:
            continue
        st = 1.0 if nm.get("strength") is None else float(nm["strength"][mat])
        uv6 = nm["tri_uv"][s.prim_shape_index[i]] if (sh["kind"] == M.TRIANGLE and nm.get("tri_uv") is not None) else None
        uv, du, dv, ok = hit_uv_and_tangents(sh, uv6, h["p"][m])
        ns, on, margin = perturb(h["ns"][m], h["ng"][m], du, dv, uv, nm["maps"][nm["mat_map"][mat]], st)
        on = on & ok
        h["uv"][m] = uv
        h["ns"][m] = np.where(on[:, None], ns, h["ns"][m]); h["perturbed"][m] = on; h["margin"][m] = np.where(ok, margin, np.inf)
    h["record"] = h["smooth"] | h["perturbed"]
    return h


def direct_delta(s, tri_vn, nm, albedo):
    """the film of a scene of matte surfaces lit by its one directional light, max_depth 1, pixel-centre rays: albedo / pi * E * |dot(Ns', wl)| where wo and
    wl lie on one side of Ns', and of the geometric normal too wherever the side record is on (the guard); (H, W, 3) float64 with (hit, fragile, mapped)
    masks.  nm None: the unmapped scene."""
    import mis_ref as M
    import normals_ref as NR
    W, H = int(s.camera.res_x), int(s.camera.res_y)
    assert s.n_lights == 1 and s.light_type[0] == M.L_DIR
    wi = -np.array([s.light_vec[k] for k in range(3)], f64)
    Li = np.array([s.light_radiance[k] for k in range(3)], f64)
    o, d = NR.camera_rays(s)
    h = mapped_hits(s, tri_vn, nm if nm is not None else dict(maps=[], mat_map=[-1] * s.n_materials), o, d)
    hit = h["prim"] >= 0
    N = h["ns"]
    wo = -d
    a_wo, a_wi = (wo * N).sum(-1), N @ wi
    g_wo, g_wi = (wo * h["ng"]).sum(-1), h["ng"] @ wi
    hemi = a_wo * a_wi > 0
    guard = np.where(h["record"], g_wo * g_wi > 0, True)
    op, _, _, _ = M.intersect(h["shapes"], h["p"], np.broadcast_to(wi, h["p"].shape))
    lit = hit & hemi & guard & (op < 0)
    L = np.where(lit[:, None], np.asarray(albedo, f64) / np.pi * Li * np.abs(a_wi)[:, None], 0.0)
    signs = np.stack([a_wo, a_wi, g_wo, g_wi], -1)
    fragile = hit & ((np.abs(signs) < 1e-4).any(-1) | (h["edge"] < 1e-4) | (h["margin"] < 1e-3))
    shp = (H, W)
    return np.clip(L, 0.0, 1.0).reshape(H, W, 3), hit.reshape(shp), fragile.reshape(shp), h["perturbed"].reshape(shp)


def map_direct_rays(s, tri_vn, nm, o, d, rgb, tint, up, through_camera=False):
    """normals_ref.map_direct_rays -- the quadrature of the direct light of a lat-long map over its texels on a convex matte mesh -- with Ns' substituted
    for Ns: that function runs unchanged on first hits whose `ns` is the mapped normal and whose `smooth` (where its guard applies) is the side record.
    -> (hit, E_ns', E_ng, texel radiance of a miss's direction), as there."""
    import normals_ref as NR
    plain = NR.first_hits

    def first_hits(s_, vn_, o_, d_, through_camera_=False):
        h = mapped_hits(s_, vn_, nm, o_, d_, through_camera_, first_hits=plain)
        h["smooth"] = h["record"]
        return h
    NR.first_hits = first_hits
    try:
        return NR.map_direct_rays(s, tri_vn, o, d, rgb, tint, up, through_camera=through_camera)
    finally:
        NR.first_hits = plain
