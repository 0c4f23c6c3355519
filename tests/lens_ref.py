"""The thin-lens camera (INTEGRATION.md "Lens") restated in float64 NumPy: the plan, the lens sample of a disk or polygonal aperture, the ray.
Inputs are the fp32 values the library receives; everything after them is float64, with one exception that is part of the definition: the polygon's
triangle selector t = u0 * (float)n is the fp32 product, because the map is discontinuous at every integer t (w = 0 is the centre, w -> 1 the edge)
and a float64 t would put a draw within an fp32 rounding of k / n into the other triangle."""
import numpy as np

f32 = np.float32


def cam_arrays(cam):
    """pos, front, right, up (float64 of the fp32 values) and the resolution of a JpCamera"""
    return tuple(np.array(list(getattr(cam, k)), np.float64) for k in ("pos", "front", "right", "up")) + (float(cam.res_x), float(cam.res_y))


def vertices(blades, rotation_deg):
    """v[k] = (cos, sin)(rotation + 2 pi k / n), k = 0 .. n, float64"""
    k = np.arange(blades + 1) % blades
    a = np.float64(f32(rotation_deg)) * (np.pi / 180.0) + 2.0 * np.pi * k / blades
    return np.stack([np.cos(a), np.sin(a)], -1)


def plan32(cam, radius, focus, blades, rotation_deg):
    """the JpLensPlan fields as the library computes them: fp32 lens axes with the length sqrtf((x*x + y*y) + z*z), vertices rounded from double"""
    out = {}
    for name, key in (("ex", "right"), ("ey", "up")):
        v = np.array(list(getattr(cam, key)), f32)
        ln = np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])))
        out[name] = (v / f32(ln)).astype(f32)
    out["v"] = vertices(blades, rotation_deg).astype(f32) if blades else np.zeros((0, 2), f32)
    out["radius"], out["focus"], out["n_verts"] = f32(radius), f32(focus), blades
    return out


def concentric_disk(u0, u1):
    ux = 2.0 * np.asarray(u0, np.float64) - 1.0; uy = 2.0 * np.asarray(u1, np.float64) - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.abs(ux) > np.abs(uy)
        r = np.where(a, ux, uy)
        th = np.where(a, (np.pi / 4) * (uy / ux), np.pi / 2 - (np.pi / 4) * (ux / uy))
    z = (ux == 0) & (uy == 0)
    th = np.where(z, 0.0, th); r = np.where(z, 0.0, r)
    return r * np.cos(th), r * np.sin(th)


def polygon_selector(u0, blades):
    """k and w of the definition: t = u0 * (float)n in fp32, k = min((int)t, n - 1), w = t - (float)k (exact)"""
    t = (np.asarray(u0, f32) * f32(blades)).astype(f32)
    k = np.minimum(t.astype(np.int64), blades - 1)
    return k, t.astype(np.float64) - k


def unit_sample(u0, u1, blades, rotation_deg, v=None):
    """the point of the unit aperture for two draws; v: the vertex table to use (default: the float64 one)"""
    if blades == 0:
        return concentric_disk(u0, u1)
    if v is None:
        v = vertices(blades, rotation_deg)
    v = np.asarray(v, np.float64)
    k, w = polygon_selector(u0, blades)
    su = np.sqrt(w)
    b = np.asarray(u1, np.float64) * su; c = su - b
    return v[k, 0] * b + v[k + 1, 0] * c, v[k, 1] * b + v[k + 1, 1] * c


def d0_of(cam, fx, fy):
    pos, front, right, up, rx, ry = cam_arrays(cam)
    a = np.asarray(fx, np.float64) / rx - 0.5; b = 0.5 - np.asarray(fy, np.float64) / ry
    return front[None] + right[None] * a[:, None] + up[None] * b[:, None]


def lens_rays(cam, radius, focus, blades, rotation_deg, fxfy, u):
    """origin, dir in float64 for fp32 film positions (n, 2) and lens draws (n, 2)"""
    pos, front, right, up, rx, ry = cam_arrays(cam)
    ex = right / np.linalg.norm(right); ey = up / np.linalg.norm(up)
    fxfy = np.asarray(fxfy, f32); u = np.asarray(u, f32)
    px, py = unit_sample(u[:, 0], u[:, 1], blades, rotation_deg)
    lx = np.float64(f32(radius)) * px; ly = np.float64(f32(radius)) * py
    off = ex[None] * lx[:, None] + ey[None] * ly[:, None]
    q = d0_of(cam, fxfy[:, 0], fxfy[:, 1]) * np.float64(f32(focus)) - off
    return pos[None] + off, q / np.linalg.norm(q, axis=-1, keepdims=True)


def pinhole_rays(cam, fxfy):
    pos = cam_arrays(cam)[0]
    fxfy = np.asarray(fxfy, f32)
    d = d0_of(cam, fxfy[:, 0], fxfy[:, 1])
    return np.tile(pos, (len(d), 1)), d / np.linalg.norm(d, axis=-1, keepdims=True)


def inside_polygon(px, py, blades, rotation_deg):
    """signed distance to the nearest edge line, positive inside (the polygon is convex and holds the origin)"""
    v = vertices(blades, rotation_deg)
    e = v[1:] - v[:-1]
    nrm = np.stack([-e[:, 1], e[:, 0]], -1); nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)      # counter-clockwise vertices: the inward normal
    d = (np.asarray(px)[:, None] - v[None, :-1, 0]) * nrm[None, :, 0] + (np.asarray(py)[:, None] - v[None, :-1, 1]) * nrm[None, :, 1]
    return d.min(-1)


def polygon_area(blades):
    return 0.5 * blades * np.sin(2.0 * np.pi / blades)


def ulp32(x):
    return float(np.spacing(f32(abs(x))))


# ---- the counter stream (include/jp_counter_rng.h) ------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
        x = x ^ (x >> np.uint32(16))
    return x


def rng_key(seed, x, y, s):
    with np.errstate(over="ignore"):
        k = mix32(np.full(np.shape(x), np.uint32(seed) ^ np.uint32(0x9E3779B9), np.uint32))
        k = mix32(k + np.asarray(x).astype(np.uint32)); k = mix32(k + np.asarray(y).astype(np.uint32)); k = mix32(k + np.asarray(s).astype(np.uint32))
    return k


def rng_float(key, dim):
    with np.errstate(over="ignore"):
        return ((mix32(key + np.uint32((dim * 0x9E3779B9) & 0xffffffff)) >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def sample_draws(seed, x, y, s, debug=False):
    """film position (n, 2) and lens draws (n, 2) of samples s of pixels (x, y): dims 0 .. 3 of the key (JP_SAMPLER_DEBUG: every draw 0.5)"""
    x = np.asarray(x); y = np.asarray(y); s = np.asarray(s)
    key = rng_key(seed, x, y, s)
    d = [np.full(x.shape, 0.5, f32) if debug else rng_float(key, k) for k in range(4)]
    fxfy = np.stack([(x.astype(f32) + d[0]).astype(f32), (y.astype(f32) + d[1]).astype(f32)], -1)
    return fxfy, np.stack([d[2], d[3]], -1)
