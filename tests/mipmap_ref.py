"""Mip maps in numpy, restated from the text of INTEGRATION.md "Mip maps" (not from the C code): the pyramid (integers), the cone's step, the world area per unit
uv area of every shape, the footprint rho and the lookup at a footprint (level and fraction from the bits of rho, trilinear between two bilinear lookups).  Every
float operation is one float32 operation in the order of the text."""
import numpy as np

import tex_sampling_ref as TR

f32 = np.float32
TWO_PI = f32(6.2831855)
TWO_PI2 = f32(19.739209)


def level_sizes(w, h):
    out = [(w, h)]
    while max(w, h) > 1:
        w, h = max(1, w >> 1), max(1, h >> 1)
        out.append((w, h))
    return out


def build_chain(img):
    """levels of an (h, w, 3) uint8 image, level 0 first"""
    levels = [np.asarray(img, np.uint8)]
    while max(levels[-1].shape[0], levels[-1].shape[1]) > 1:
        s = levels[-1].astype(np.int64); sh, sw, _ = s.shape
        dw, dh = max(1, sw >> 1), max(1, sh >> 1)
        i = np.arange(dw); j = np.arange(dh)
        i0 = np.minimum(2 * i, sw - 1); i1 = np.minimum(2 * i + 1, sw - 1); j0 = np.minimum(2 * j, sh - 1); j1 = np.minimum(2 * j + 1, sh - 1)
        d = (s[j0][:, i0] + s[j0][:, i1] + s[j1][:, i0] + s[j1][:, i1] + 2) >> 2
        levels.append(d.astype(np.uint8))
    return levels


def cone_step(gamma0, bounce_spread, flags, t, state):
    """one hit per cone: state (n, 2) (width, spread) -> the state after"""
    flags = np.asarray(flags, np.int64); t = np.asarray(t, f32); st = np.array(state, f32).reshape(-1, 2)
    g = f32(gamma0); bs = f32(bounce_spread)
    with np.errstate(all="ignore"):
        first = (flags & 0xff) == 0
        spec = ((flags >> 8) & 1) == 1
        spread = np.where(first, g, np.where(spec, st[:, 1], np.where(st[:, 1] > bs, st[:, 1], bs))).astype(f32)
        step = (spread * t).astype(f32)
        width = np.where(first, step, (st[:, 0] + step).astype(f32)).astype(f32)
    return np.stack([width, spread], -1).astype(f32)


def _cross_len(a, b):
    x = ((a[:, 1] * b[:, 2]).astype(f32) - (a[:, 2] * b[:, 1]).astype(f32)).astype(f32)
    y = ((a[:, 2] * b[:, 0]).astype(f32) - (a[:, 0] * b[:, 2]).astype(f32)).astype(f32)
    z = ((a[:, 0] * b[:, 1]).astype(f32) - (a[:, 1] * b[:, 0]).astype(f32)).astype(f32)
    return np.sqrt((((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)).astype(f32)


def area_triangle(p0, p1, p2, uv6):
    p0, p1, p2, uv6 = (np.asarray(a, f32).reshape(-1, k) for a, k in ((p0, 3), (p1, 3), (p2, 3), (uv6, 6)))
    du1 = (uv6[:, 2] - uv6[:, 0]).astype(f32); dv1 = (uv6[:, 3] - uv6[:, 1]).astype(f32); du2 = (uv6[:, 4] - uv6[:, 0]).astype(f32); dv2 = (uv6[:, 5] - uv6[:, 1]).astype(f32)
    with np.errstate(all="ignore"):
        det = ((du1 * dv2).astype(f32) - (dv1 * du2).astype(f32)).astype(f32)
        a = (_cross_len((p1 - p0).astype(f32), (p2 - p0).astype(f32)) / np.abs(det)).astype(f32)
    return np.where((det == 0) | ~np.isfinite(det), f32(0), a).astype(f32)


def area_rectangle(p0, p1, p3):
    p0, p1, p3 = (np.asarray(a, f32).reshape(-1, 3) for a in (p0, p1, p3))
    return _cross_len((p1 - p0).astype(f32), (p3 - p0).astype(f32))


def area_sphere(d, radius):
    d = np.asarray(d, f32).reshape(-1, 3)
    return ((TWO_PI2 * f32(radius)).astype(f32) * np.sqrt(((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)).astype(f32)).astype(f32)


def area_disk(v0, radius):
    v = np.asarray(v0, f32).reshape(-1, 3)
    l2 = (((v[:, 0] * v[:, 0]).astype(f32) + (v[:, 1] * v[:, 1]).astype(f32)).astype(f32) + (v[:, 2] * v[:, 2]).astype(f32)).astype(f32)
    return ((TWO_PI * f32(radius)).astype(f32) * np.sqrt(l2).astype(f32)).astype(f32)


def rho(width, area, w, h, scale=(1.0, 1.0), footprint_scale=1.0):
    width = np.asarray(width, f32); area = np.asarray(area, f32)
    with np.errstate(all="ignore"):
        k = ((f32(w) * f32(scale[0])).astype(f32) * (f32(h) * f32(scale[1])).astype(f32)).astype(f32)
        r = ((width * np.sqrt((k / area).astype(f32)).astype(f32)).astype(f32) * f32(footprint_scale)).astype(f32)
        ok = (area > 0) & np.isfinite(area) & np.isfinite(r)
    return np.where(ok, r, f32(0)).astype(f32)


def gamma0(up, res_y):
    up = np.asarray(up, f32)
    l = np.sqrt((((up[0] * up[0]).astype(f32) + (up[1] * up[1]).astype(f32)).astype(f32) + (up[2] * up[2]).astype(f32)).astype(f32)).astype(f32)
    return ((f32(2) * l).astype(f32) / f32(res_y)).astype(f32)


def _bilinear_float(s, lev, u, v):
    h, w, _ = lev.shape
    i0, i1, j0, j1, fx, fy = TR._taps(s, w, h, u, v)
    F = lev.astype(f32)
    return TR._lerp(F[j0, i0], F[j0, i1], F[j1, i0], F[j1, i1], fx[:, None], fy[:, None])


def _quant(r):
    return np.minimum((r + f32(0.5)).astype(f32).astype(np.int64), 255).astype(np.uint8)


def lookup(s, img, uv, rho_):
    """a colour texture under the record s (None: none) at footprints rho_ -> (n, 3) uint8"""
    img = np.asarray(img, np.uint8)
    uv = np.asarray(uv, f32).reshape(-1, 2); r = np.asarray(rho_, f32)
    out = TR.lookup(s, img, uv)                                       # rho <= 1, and every rho that is not finite
    with np.errstate(all="ignore"):
        above = (r > 1) & np.isfinite(r)
    if not above.any():
        return out
    levels = build_chain(img); L = len(levels)
    sa = s if (s is not None and not s.identity()) else TR.Sampler()
    u, v = TR._uv(sa, uv)
    bits = r.view(np.uint32).astype(np.int64)
    l = ((bits >> 23) & 0xff) - 127
    l = np.where(above, np.minimum(l, L - 1), -1)
    for lk in np.unique(l[above]):
        k = np.nonzero(l == lk)[0]; lk = int(lk)
        if lk >= L - 1:
            out[k] = _quant(_bilinear_float(sa, levels[L - 1], u[k], v[k]))
            continue
        f = ((r[k] * f32(2.0 ** -lk)).astype(f32) - f32(1)).astype(f32)[:, None]
        ra = _bilinear_float(sa, levels[lk], u[k], v[k]); rb = _bilinear_float(sa, levels[lk + 1], u[k], v[k])
        out[k] = _quant((ra + (f * (rb - ra).astype(f32)).astype(f32)).astype(f32))
    return out
