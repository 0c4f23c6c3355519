"""Environment maps restated in float64 numpy from the definition of INTEGRATION.md "Environment maps" -- weights, texel records, lookup, sample,
the map light's weight and the closed form of a matte floor under the map.  Written from the text, not from the C++: the tests compare the library
against this file.  The alias table itself is jp.build_light_table's (tests/test_light_table_host.py has its checklist); sample() takes it as input."""
import numpy as np

f32 = np.float32
UP_Z, UP_Y = 0, 1


def row_cos(H):
    """(ct_r, cb_r) = (cos(pi r / H), cos(pi (r + 1) / H)) per row, float64"""
    r = np.arange(H, dtype=np.float64)
    return np.cos(np.pi * r / H), np.cos(np.pi * (r + 1) / H)


def omega(W, H):
    """solid angle of one texel of each row: (2 pi / W) (ct_r - cb_r)"""
    ct, cb = row_cos(H)
    return (2.0 * np.pi / W) * (ct - cb)


def tinted(rgb, tint):
    """the device texel: the fp32 product tint x texel per channel, (H, W, 3) float32"""
    return (np.asarray(rgb, f32) * np.asarray(tint, f32)[None, None, :]).astype(f32)


def weights(rgb, tint, importance=0):
    """w_t in row-major order (float64), from the tinted fp32 values; importance -1: the solid angle alone"""
    t = tinted(rgb, tint).astype(np.float64)
    H, W = t.shape[:2]
    om = omega(W, H)[:, None]
    if importance == -1:
        return np.broadcast_to(om, (H, W)).reshape(-1).copy()
    return (((t[..., 0] + t[..., 1]) + t[..., 2]) * om).reshape(-1)


def total(w):
    """W_env: the weights summed in index order"""
    return float(np.cumsum(np.asarray(w, np.float64))[-1])


def texel_pdf(w, W, H):
    """pdf_t = (w_t / W_env) / Omega_r in float64 (the device holds its fp32 rounding); all 0 for an all-black map"""
    w = np.asarray(w, np.float64)
    Wenv = total(w)
    if Wenv == 0.0:
        return np.zeros_like(w)
    return (w / Wenv) / np.repeat(omega(W, H), W)


def mean_sum(rgb, tint):
    """S = sum_t (R + G + B)_t Omega_r / (4 pi)"""
    return total(weights(rgb, tint, 0)) / (4.0 * np.pi)


def light_weight(rgb, tint, world_radius):
    """the map light's weight in the light table: (S pi) R^2"""
    return (mean_sum(rgb, tint) * np.pi) * (float(world_radius) * float(world_radius))


def to_map(d, up):
    """world direction -> map space: UP_Z the identity, UP_Y map (x, y, z) = world (z, x, y)"""
    d = np.asarray(d)
    return d[..., [2, 0, 1]] if up == UP_Y else d


def to_world(m, up):
    m = np.asarray(m)
    return m[..., [1, 2, 0]] if up == UP_Y else m


def texel_coords(d, W, H, up):
    """float64 texel coordinates (row, col) of world directions: theta H / pi, phi W / 2 pi with phi in [0, 2 pi)"""
    m = to_map(np.asarray(d, np.float64), up)
    m = m / np.linalg.norm(m, axis=-1, keepdims=True)
    theta = np.arccos(np.clip(m[..., 2], -1.0, 1.0))
    phi = np.arctan2(m[..., 1], m[..., 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    return theta * (H / np.pi), phi * (W / (2.0 * np.pi))


def lookup(d, W, H, up):
    """-> (texel index, distance of the nearer coordinate to a texel border in texel units)"""
    fr, fc = texel_coords(d, W, H, up)
    row = np.minimum(fr.astype(np.int64), H - 1); col = np.minimum(fc.astype(np.int64), W - 1)
    border = np.minimum(np.abs(fr - np.round(fr)), np.abs(fc - np.round(fc)))
    return row * W + col, border


def sample(u, q, alias, W, H, up):
    """the five draws a0 a1 a2 b0 b1 (fp32, (n, 5)) -> (texel index j, world-space wi float64).  The index uses the fp32 products the definition
    names; the direction is evaluated in float64 from the fp32 row cosines the device holds."""
    u = np.asarray(u, f32).reshape(-1, 5)
    a0, a1, a2, b0, b1 = (u[:, k] for k in range(5))
    r0 = np.minimum((a0 * f32(H)).astype(np.int64), H - 1)
    c0 = np.minimum((a1 * f32(W)).astype(np.int64), W - 1)
    i = r0 * W + c0
    j = np.where(a2 < np.asarray(q, f32)[i], i, np.asarray(alias, np.int64)[i])
    r, c = j // W, j % W
    ct, cb = row_cos(H)
    ct = ct.astype(f32).astype(np.float64)[r]; cb = cb.astype(f32).astype(np.float64)[r]
    cos_t = ct - b1.astype(np.float64) * (ct - cb)
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = (c + b0.astype(np.float64)) * (2.0 * np.pi / W)
    m = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], -1)
    return j, to_world(m, up)


def floor_closed_form(rgb, tint, kd):
    """radiance leaving a matte floor (albedo kd) whose normal is the map's up axis, lit by the whole map and nothing else:
    kd / pi * sum_t L_t (2 pi / W) (max(ct, 0)^2 - max(cb, 0)^2) / 2 -- the integral of cos(theta) over each texel of the upper hemisphere"""
    t = tinted(rgb, tint).astype(np.float64)
    H, W = t.shape[:2]
    ct, cb = row_cos(H)
    g = (2.0 * np.pi / W) * (np.maximum(ct, 0.0) ** 2 - np.maximum(cb, 0.0) ** 2) / 2.0
    return np.asarray(kd, np.float64) / np.pi * (t * g[:, None, None]).sum((0, 1))


def bright_map(scale=1.0):
    """the 16 x 8 map of the tests: a dim sky gradient, two bright texels above the horizon, one below, one black row (row 6)"""
    H, W = 8, 16
    m = np.zeros((H, W, 3), np.float64)
    for r in range(H):
        m[r] = np.array([0.05, 0.07, 0.10]) * (1.0 + 0.25 * r) + 0.01 * np.arange(W)[:, None] * np.array([1.0, 0.5, 0.25])
    m[6] = 0.0
    m[1, 3] = (40.0, 30.0, 20.0)      # above the horizon
    m[2, 11] = (25.0, 20.0, 18.0)
    m[5, 7] = (30.0, 30.0, 30.0)      # below it
    return (m * scale).astype(f32)
