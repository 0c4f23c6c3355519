"""The estimator of INTEGRATION.md "Estimator" restated in float64 numpy -- the light strategy's pdf for every light kind, the power-heuristic weight,
Lambert's polygon formula for a one-sided rectangle light, a small ray caster for the probe scenes, and a single-point Monte-Carlo restatement of both
estimators (next-event estimation alone, and next-event estimation with the BSDF sample weighted against it).  Written from the text, not from the
C++: the tests compare the library against this file.  The map light reuses tests/envmap_ref.py; the light table's pmf is an input (its builder has
its own tests)."""
import functools

import numpy as np

import envmap_ref as E

TRIANGLE, RECTANGLE, SPHERE, DISK = 0, 1, 2, 3
L_ENV, L_AREA, L_POINT, L_DIR = 0, 1, 2, 3


# ---- the scene as the library receives it -------------------------------------------------------------------------------------------------
def shapes_of(s):
    """the primitives of a flattened scene (JpScene) as dicts in float64: kind, geometry, light index"""
    def v(ptr, i, n=3):
        return np.array([ptr[n * i + k] for k in range(n)], np.float64)
    out = []
    for i in range(s.n_primitives):
        k, j = s.prim_shape_type[i], s.prim_shape_index[i]
        d = dict(kind=k, light=s.prim_light[i])
        if k == TRIANGLE:
            d.update(p0=v(s.tri_p0, j), p1=v(s.tri_p1, j), p2=v(s.tri_p2, j), n=v(s.tri_n, j))
            d["area"] = 0.5 * np.linalg.norm(np.cross(d["p1"] - d["p0"], d["p2"] - d["p0"]))
        elif k == RECTANGLE:
            d.update(p0=v(s.rect_p0, j), p1=v(s.rect_p1, j), p2=v(s.rect_p2, j), p3=v(s.rect_p3, j), n=v(s.rect_n, j))
            d["area"] = np.linalg.norm(d["p0"] - d["p1"]) * np.linalg.norm(d["p2"] - d["p1"])
        elif k == SPHERE:
            d.update(c=v(s.sph_center, j), r=float(s.sph_radius[j]))
            d["area"] = 4.0 * np.pi * d["r"] ** 2
        else:
            d.update(c=v(s.disk_center, j), n=v(s.disk_normal, j), r=float(s.disk_radius[j]))
            d["area"] = np.pi * d["r"] ** 2
        out.append(d)
    return out


def lights_of(s):
    """the lights of a flattened scene: kind, radiance, emitting primitive"""
    return [dict(kind=s.light_type[i], radiance=np.array([s.light_radiance[3 * i + k] for k in range(3)], np.float64), prim=s.light_prim[i])
            for i in range(s.n_lights)]


def intersect(shapes, o, d, tmin=1e-3):
    """closest hit of the rays (o, d) (n, 3) with the shapes -> (primitive index or -1, t, |cos| of the ray at the hit, the hit emits toward the origin).
    Rectangles face whoever looks at them (shape.h:427); triangles, disks and spheres emit on the side of their normal."""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    n = o.shape[0]
    best = np.full(n, np.inf); prim = np.full(n, -1); cosb = np.zeros(n); front = np.zeros(n, bool)
    for i, sh in enumerate(shapes):
        if sh["kind"] == SPHERE:
            oc = o - sh["c"]
            b = (oc * d).sum(-1); c = (oc * oc).sum(-1) - sh["r"] ** 2
            disc = b * b - c
            ok = disc > 0
            sq = np.sqrt(np.where(ok, disc, 0.0))
            t = np.where(-b - sq > tmin, -b - sq, -b + sq)
            ok &= t > tmin
            p = o + t[:, None] * d
            nn = (p - sh["c"]) / sh["r"]
            cs = (nn * d).sum(-1); fr = cs < 0
        else:
            nrm = sh["n"]; p0 = sh["c"] if sh["kind"] == DISK else sh["p1"] if sh["kind"] == RECTANGLE else sh["p0"]
            den = (d * nrm).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((p0 - o) * nrm).sum(-1) / den
            ok = np.isfinite(t) & (t > tmin)
            p = o + np.where(ok, t, 0.0)[:, None] * d
            if sh["kind"] == DISK:
                ok &= ((p - sh["c"]) ** 2).sum(-1) <= sh["r"] ** 2
            elif sh["kind"] == RECTANGLE:
                e0, e1 = sh["p0"] - sh["p1"], sh["p2"] - sh["p1"]
                a = ((p - sh["p1"]) * e0).sum(-1) / (e0 * e0).sum(); b = ((p - sh["p1"]) * e1).sum(-1) / (e1 * e1).sum()
                ok &= (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
            else:
                e0, e1 = sh["p1"] - sh["p0"], sh["p2"] - sh["p0"]
                w = p - sh["p0"]
                d00, d01, d11 = (e0 * e0).sum(), (e0 * e1).sum(), (e1 * e1).sum()
                w0, w1 = (w * e0).sum(-1), (w * e1).sum(-1)
                den2 = d00 * d11 - d01 * d01
                a = (d11 * w0 - d01 * w1) / den2; b = (d00 * w1 - d01 * w0) / den2
                ok &= (a >= 0) & (b >= 0) & (a + b <= 1)
            cs = den; fr = (den < 0) | (sh["kind"] == RECTANGLE)
        take = ok & (t < best)
        best = np.where(take, t, best); prim = np.where(take, i, prim); cosb = np.where(take, np.abs(cs), cosb); front = np.where(take, fr, front)
    return prim, best, cosb, front


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def weight(own, other):
    """power heuristic, exponent 2: the weight of the strategy with pdf `own` against the one with pdf `other`"""
    own = np.asarray(own, np.float64); other = np.asarray(other, np.float64)
    r = other / own
    return 1.0 / (1.0 + r * r)


def usable(a):
    a = np.asarray(a, np.float64)
    return np.where(np.isfinite(a) & (a > 0), a, 0.0)


def light_pdf_area(sh, pmf, p, d, dist, cos_light):
    """a = pmf * pdf_Li for the emitting shape sh reached from p along d after dist, |cos| at the light cos_light; 0 inside a sphere light"""
    p = np.asarray(p, np.float64)
    if sh["kind"] == SPHERE:
        d2 = ((p - sh["c"]) ** 2).sum(-1)
        inside = d2 <= sh["r"] ** 2
        cos_max = np.sqrt(np.maximum(0.0, 1.0 - sh["r"] ** 2 / np.where(inside, 1.0, d2)))
        with np.errstate(divide="ignore"):
            return np.where(inside, 0.0, usable(pmf / (2.0 * np.pi * (1.0 - cos_max))))
    with np.errstate(divide="ignore", invalid="ignore"):
        return usable(pmf * (1.0 / sh["area"]) * (np.asarray(dist, np.float64) ** 2 / cos_light))


def light_pdf_constant(pmf, d):
    """a constant environment light: uniform in (theta, phi) about the world's z axis"""
    d = np.asarray(d, np.float64)
    with np.errstate(divide="ignore"):
        return usable(pmf / (2.0 * np.pi ** 2 * np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)))


def light_pdf_map(pmf, d, rgb, tint, up, importance=0):
    """the map light: pmf * the pdf of the texel the direction sees -> (a, distance to the nearest texel border in texel units)"""
    H, W = np.asarray(rgb).shape[:2]
    idx, border = E.lookup(d, W, H, up)
    return usable(pmf * E.texel_pdf(E.weights(rgb, tint, importance), W, H)[idx]), border


def light_pdf(shapes, lights, pmf, o, d, env=None):
    """jp_light_pdf restated: rays (o, d) -> (light reached or -1, a, |cos| at the light or 1, texel-border distance or 1, 1 - cos_max of a sphere
    light or 1).  The last three say how well conditioned the fp32 evaluation is: the division by |cos|, the (int) of a texel coordinate, the
    subtraction 1 - cos_max.  env: dict(rgb, tint, up) when the scene's environment light is a map."""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    prim, t, cosl, front = intersect(shapes, o, d)
    n = o.shape[0]
    light = np.full(n, -1); a = np.zeros(n); border = np.ones(n); cos_out = np.ones(n); cone = np.ones(n)
    for i, sh in enumerate(shapes):
        m = (prim == i) & front & (sh["light"] >= 0)
        if not m.any() or not lights[sh["light"]]["radiance"].any():
            continue
        light[m] = sh["light"]; cos_out[m] = cosl[m]
        a[m] = light_pdf_area(sh, float(pmf[sh["light"]]), o[m], d[m], t[m], cosl[m])
        if sh["kind"] == SPHERE:
            cone[m] = 1.0 - np.sqrt(np.maximum(0.0, 1.0 - sh["r"] ** 2 / ((o[m] - sh["c"]) ** 2).sum(-1)))
    miss = prim < 0
    envs = [i for i, l in enumerate(lights) if l["kind"] == L_ENV and l["radiance"].any()]
    if miss.any() and envs:
        li = envs[0]
        light[miss] = li
        if env is not None:
            a[miss], border[miss] = light_pdf_map(float(pmf[li]), d[miss], env["rgb"], env["tint"], env["up"])
        else:
            a[miss] = light_pdf_constant(float(pmf[li]), d[miss])
    return light, a, cos_out, border, cone


# ---- closed form: Lambert's polygon formula ---------------------------------------------------------------------------------------------------------
def polygon_irradiance(verts, p, n):
    """irradiance / radiance at points p (m, 3) with normal n of a polygon (k, 3) that lies wholly above the plane of p and faces it:
    1/2 sum_i angle(v_i, v_i+1) * dot(n, unit(v_i x v_i+1)), as a positive number"""
    p = np.asarray(p, np.float64); verts = np.asarray(verts, np.float64); n = np.asarray(n, np.float64)
    v = verts[None, :, :] - p[:, None, :]
    v = v / np.linalg.norm(v, axis=-1, keepdims=True)
    w = np.roll(v, -1, axis=1)
    ang = np.arccos(np.clip((v * w).sum(-1), -1.0, 1.0))
    c = np.cross(v, w)
    c = c / np.linalg.norm(c, axis=-1, keepdims=True)
    return np.abs(0.5 * (ang * (c @ n)).sum(-1))


def rect_corners(sh):
    return np.array([sh["p0"], sh["p1"], sh["p2"], sh["p2"] + sh["p0"] - sh["p1"]])


# ---- BSDFs (local frame, z the normal) ------------------------------------------------------------------------------------------------------
def tr_D(wh, al):
    c2 = wh[..., 2] ** 2
    t2 = (1.0 - c2) / c2
    return 1.0 / (np.pi * al * al * c2 * c2 * (1.0 + t2 / (al * al)) ** 2)


def tr_lambda(w, al):
    c2 = w[..., 2] ** 2
    t2 = np.maximum(0.0, 1.0 - c2) / c2
    return (-1.0 + np.sqrt(1.0 + al * al * t2)) / 2.0


def fresnel_conductor(cos_i, eta, k):
    c2 = cos_i * cos_i; s2 = 1.0 - c2
    e2, k2 = eta * eta, k * k
    t0 = e2 - k2 - s2
    a2b2 = np.sqrt(t0 * t0 + 4.0 * e2 * k2)
    t1 = a2b2 + c2
    a = np.sqrt(0.5 * (a2b2 + t0))
    t2 = 2.0 * a * cos_i
    rs = (t1 - t2) / (t1 + t2)
    t3 = c2 * a2b2 + s2 * s2
    t4 = t2 * s2
    rp = rs * (t3 - t4) / (t3 + t4)
    return 0.5 * (rp + rs)


def metal_f(wo, wi, al, eta, k):
    """isotropic Trowbridge-Reitz conductor, one channel: D G F / (4 cos cos); 0 across the surface"""
    wh = wo + wi
    wh = wh / np.linalg.norm(wh, axis=-1, keepdims=True)
    G = 1.0 / (1.0 + tr_lambda(wo, al) + tr_lambda(wi, al))
    F = fresnel_conductor(np.abs((wi * wh).sum(-1)), eta, k)
    f = tr_D(wh, al) * G * F / (4.0 * np.abs(wi[..., 2]) * np.abs(wo[..., 2]))
    return np.where(wi[..., 2] * wo[..., 2] > 0, f, 0.0)


def metal_pdf(wo, wi, al):
    """the pdf of sampling the visible normals and reflecting: D G1(wo) |wo.wh| / |wo.z| / (4 wo.wh)"""
    wh = wo + wi
    wh = wh / np.linalg.norm(wh, axis=-1, keepdims=True)
    owh = (wo * wh).sum(-1)
    p = tr_D(wh, al) / (1.0 + tr_lambda(wo, al)) * np.abs(owh) / np.abs(wo[..., 2]) / (4.0 * owh)
    return np.where(wi[..., 2] * wo[..., 2] > 0, p, 0.0)


def metal_sample(wo, al, u0, u1):
    """a direction with density metal_pdf: the visible-normal distribution sampled by stretching, a disk sample and unstretching"""
    vh = np.array([al * wo[0], al * wo[1], wo[2]]); vh = vh / np.linalg.norm(vh)
    lensq = vh[0] ** 2 + vh[1] ** 2
    t1 = np.array([-vh[1], vh[0], 0.0]) / np.sqrt(lensq) if lensq > 0 else np.array([1.0, 0.0, 0.0])
    t2 = np.cross(vh, t1)
    r = np.sqrt(u0); phi = 2.0 * np.pi * u1
    a = r * np.cos(phi); b = r * np.sin(phi)
    s = 0.5 * (1.0 + vh[2])
    b = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - a * a)) + s * b
    nh = a[:, None] * t1 + b[:, None] * t2 + np.sqrt(np.maximum(0.0, 1.0 - a * a - b * b))[:, None] * vh
    wh = np.stack([al * nh[:, 0], al * nh[:, 1], np.maximum(0.0, nh[:, 2])], -1)
    wh = wh / np.linalg.norm(wh, axis=-1, keepdims=True)
    return 2.0 * (wh @ wo)[:, None] * wh - wo


# ---- single-point Monte Carlo of both estimators --------------------------------------------------------------------------------------------------
def point_estimators(corners, light_n, Le, p, frame, bsdf, n=10 ** 6, seed=5):
    """Direct light at the point p (shading frame (s, t, n) as rows of `frame`) from one one-sided rectangle light (corner p1 = corners[1] with edges to
    corners[0] and corners[2], normal light_n, radiance Le, selection probability 1, nothing in between), estimated n times by
      nee: one point on the light, f Le cos / p_light
      mis: that sample weighted against the BSDF's pdf for it, plus one BSDF sample weighted against the light's pdf for it where it reaches the light.
    bsdf: dict(f(wo, wi), pdf(wo, wi), sample(wo, u0, u1), wo).  -> dict(nee=(mean, per-sample variance), mis=(mean, per-sample variance))"""
    rng = np.random.default_rng(seed)
    corners = np.asarray(corners, np.float64); p = np.asarray(p, np.float64); frame = np.asarray(frame, np.float64)
    e0, e1 = corners[0] - corners[1], corners[2] - corners[1]
    area = np.linalg.norm(e0) * np.linalg.norm(e1)
    wo = bsdf["wo"]
    u = rng.random((n, 4))
    # the light strategy
    lp = corners[1] + u[:, :1] * e0 + u[:, 1:2] * e1
    v = lp - p
    d2 = (v * v).sum(-1); wi_w = v / np.sqrt(d2)[:, None]
    cl = -(wi_w @ light_n)
    wi = wi_w @ frame.T
    pl = np.where(cl > 0, d2 / (area * np.maximum(cl, 1e-300)), np.inf)
    fl = np.where((cl > 0) & (wi[:, 2] > 0), bsdf["f"](wo, wi) * Le * np.abs(wi[:, 2]) / pl, 0.0)
    nee = fl
    wl = np.where(fl > 0, weight(pl, bsdf["pdf"](wo, wi)), 0.0)
    # the BSDF strategy
    wb = bsdf["sample"](wo, u[:, 2], u[:, 3])
    wb_w = wb @ frame
    den = wb_w @ light_n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((corners[1] - p) @ light_n) / den
    hit = np.isfinite(t) & (t > 0) & (den < 0) & (wb[:, 2] > 0)
    q = p + np.where(hit, t, 0.0)[:, None] * wb_w - corners[1]
    a = (q @ e0) / (e0 @ e0); b = (q @ e1) / (e1 @ e1)
    hit &= (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    pb = bsdf["pdf"](wo, wb)
    hit &= pb > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pl_b = np.where(hit, t * t / (area * np.maximum(-den, 1e-300)), 0.0)
        fb = np.where(hit, bsdf["f"](wo, wb) * Le * np.abs(wb[:, 2]) / pb * weight(pb, pl_b), 0.0)
    mis = fl * wl + fb
    return dict(nee=(float(nee.mean()), float(nee.var(ddof=1))), mis=(float(mis.mean()), float(mis.var(ddof=1))))


def lambert_bsdf(kd):
    def sample(wo, u0, u1):
        r = np.sqrt(u0); phi = 2.0 * np.pi * u1
        return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u0))], -1)
    return dict(wo=np.array([0.0, 0.0, 1.0]), f=lambda wo, wi: np.where(wi[..., 2] > 0, kd / np.pi, 0.0),
                pdf=lambda wo, wi: np.where(wi[..., 2] > 0, wi[..., 2] / np.pi, 0.0), sample=sample)


def metal_bsdf(wo, al, eta, k):
    wo = np.asarray(wo, np.float64) / np.linalg.norm(wo)
    return dict(wo=wo, f=lambda o, wi: metal_f(o, wi, al, eta, k), pdf=lambda o, wi: metal_pdf(o, wi, al), sample=lambda o, u0, u1: metal_sample(o, al, u0, u1))


# ---- the scenes of the variance tests (tests/test_mis_host.py fixes their parameters, tests/test_gpu_mis.py renders them) ---------------------------
LAMP = dict(half=1.0, height=0.05, kd=0.8, Le=0.08)                   # a matte floor `height` below a lamp of 2 half x 2 half, facing down
METAL = dict(alpha=0.02, eta=0.2, k=3.9, eta3=(0.2, 0.9, 1.1), k3=(3.9, 2.4, 2.2), Le=0.1,
             eye=(5.0, 2.0, 0.0), light_x=-5.0, light_y=(0.0, 4.0), light_z=(-2.0, 2.0))   # a metal floor, the eye at the mirror angle to a 4 x 4 light


@functools.lru_cache(maxsize=None)
def lamp_prediction(x=0.0, z=0.0, n=10 ** 6):
    h, a = LAMP["height"], LAMP["half"]
    corners = np.array([[a, h, -a], [-a, h, -a], [-a, h, a]])
    frame = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    return point_estimators(corners, np.array([0.0, -1.0, 0.0]), LAMP["Le"], np.array([x, 0.0, z]), frame, lambert_bsdf(LAMP["kd"]), n)


def lamp_closed_form(x=0.0, z=0.0):
    h, a = LAMP["height"], LAMP["half"]
    verts = np.array([[a, h, -a], [-a, h, -a], [-a, h, a], [a, h, a]])
    return float(LAMP["kd"] / np.pi * LAMP["Le"] * polygon_irradiance(verts, np.array([[x, 0.0, z]]), np.array([0.0, 1.0, 0.0]))[0])


@functools.lru_cache(maxsize=None)
def metal_prediction(n=10 ** 6):
    m = METAL
    corners = np.array([[m["light_x"], m["light_y"][1], m["light_z"][0]], [m["light_x"], m["light_y"][0], m["light_z"][0]], [m["light_x"], m["light_y"][0], m["light_z"][1]]])
    frame = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    wo = frame @ np.asarray(m["eye"])
    return point_estimators(corners, np.array([1.0, 0.0, 0.0]), m["Le"], np.zeros(3), frame, metal_bsdf(wo, m["alpha"], m["eta"], m["k"]), n)
