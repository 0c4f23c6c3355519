"""The variance definitions (INTEGRATION.md "Variance") restated in numpy float32, independent of the library: the running moments of a pixel's sample
luminances (moments_ref) and the variance-guided a-trous filter (atrous_v_ref), vectorised over pixels, every operation one float32 operation in the order
written.  Shared by test_variance_host.py (CPU) and test_gpu_variance.py."""
import numpy as np

from denoise_ref import H5, _sq3, filter_inputs  # noqa: F401  (filter_inputs: re-exported for the tests)

f32 = np.float32
K3 = np.array([0.25, 0.5, 0.25], f32)
WR, WG, WB = f32(0.2126), f32(0.7152), f32(0.0722)


def _lum(rgb):
    return ((WR * rgb[..., 0]).astype(f32) + (WG * rgb[..., 1]).astype(f32)).astype(f32) + (WB * rgb[..., 2]).astype(f32)


def clamp_samples_ref(c, rgb):
    """jp_film_clamp_sample with clamp c > 0 on (..., 3) samples"""
    rgb = np.asarray(rgb, f32)
    bad = ~np.isfinite(rgb).all(-1)
    safe = np.where(bad[..., None], f32(0), rgb).astype(f32)
    m = np.maximum(np.maximum(safe[..., 0], safe[..., 1]), safe[..., 2])           # (finite values: the order of the comparisons does not matter)
    over = m > f32(c)
    k = (f32(c) / np.where(over, m, f32(1))).astype(f32)
    return np.where(over[..., None], (safe * k[..., None]).astype(f32), safe).astype(f32)


def moments_ref(samples, sample_clamp=0.0):
    """(spp, n, 3) float32 samples in sample order -> (variance (n,), mean (n,)): Welford's recurrence on the luminances, then (m2 / (spp - 1)) / spp"""
    s = np.asarray(samples, f32)
    spp, n = s.shape[:2]
    assert spp >= 2
    if sample_clamp > 0:
        s = clamp_samples_ref(sample_clamp, s)
    mean = np.zeros(n, f32); m2 = np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            y = _lum(s[k]).astype(f32)
            y = np.where(np.isfinite(y), y, f32(0)).astype(f32)
            d = (y - mean).astype(f32)
            mean = (mean + (d / f32(k + 1)).astype(f32)).astype(f32)
            m2 = (m2 + (d * (y - mean).astype(f32)).astype(f32)).astype(f32)
        var = ((m2 / f32(spp - 1)).astype(f32) / f32(spp)).astype(f32)
    return var, mean


def atrous_v_ref(film, albedo, normal, depth, variance, iterations=5, sigma_color=8.0, sigma_normal=0.1, sigma_depth=0.03, demodulate=True, hdr=False):
    """(H, W, 3) film, albedo, normal; (H, W) depth, variance -> ((H, W, 3) out, (H, W) variance_out), float32"""
    film = np.asarray(film, f32); normal = np.asarray(normal, f32); z = np.asarray(depth, f32)
    Hh, W = z.shape
    a = np.maximum(np.asarray(albedo, f32), f32(0.001)).astype(f32) if demodulate else np.ones_like(film)
    c = (film / a).astype(f32)
    aY = _lum(a).astype(f32)
    aY2 = (aY * aY).astype(f32)
    vin = np.asarray(variance, f32)
    vin = np.where(np.isnan(vin), f32(0), vin).astype(f32)                           # v > 0 ? min(v, 1e30f) : 0 -- a NaN compares false
    vin = np.where(vin > 0, np.minimum(vin, f32(1e30)), f32(0)).astype(f32)
    v = (vin / aY2).astype(f32)
    sc, sn, sz = f32(sigma_color), f32(sigma_normal), f32(sigma_depth)
    kn = f32(1) / (sn * sn); kz = f32(1) / (sz * sz); sc2 = sc * sc
    one = f32(1)
    for i in range(iterations):
        s = 1 << i
        gs = np.zeros((Hh, W), f32); ks = np.zeros((Hh, W), f32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                y0, y1 = max(0, -dy), min(Hh, Hh - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                k3 = f32(K3[dy + 1] * K3[dx + 1])
                gs[P] = (gs[P] + (k3 * v[Q]).astype(f32)).astype(f32)
                ks[P] = (ks[P] + k3).astype(f32)
        g = (gs / ks).astype(f32)
        kc = (one / ((sc2 * g).astype(f32) + f32(1e-8)).astype(f32)).astype(f32)
        num = np.zeros_like(c); den = np.zeros((Hh, W), f32); vnum = np.zeros((Hh, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                y0, y1 = max(0, -oy), min(Hh, Hh - oy)            # pixels p whose tap q = p + (ox, oy) is inside the image
                x0, x1 = max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                hh = f32(H5[dy + 2] * H5[dx + 2])
                dc = _sq3((c[P] - c[Q]).astype(f32))
                dn = _sq3((normal[P] - normal[Q]).astype(f32))
                m = np.maximum(np.maximum(z[P], z[Q]), f32(1e-20)).astype(f32)
                rz = ((z[P] - z[Q]).astype(f32) / m).astype(f32)
                dz = (rz * rz).astype(f32)
                w = (hh / (((one + (dc * kc[P]).astype(f32)).astype(f32) * (one + (dn * kn).astype(f32)).astype(f32)).astype(f32)
                           * (one + (dz * kz).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                num[P] = (num[P] + (w[..., None] * c[Q]).astype(f32)).astype(f32)
                den[P] = (den[P] + w).astype(f32)
                vnum[P] = (vnum[P] + ((w * w).astype(f32) * v[Q]).astype(f32)).astype(f32)
        c = (num / den[..., None]).astype(f32)
        v = (vnum / (den * den).astype(f32)).astype(f32)
    out = np.maximum((c * a).astype(f32), f32(0)).astype(f32)
    if not hdr:
        out = np.minimum(out, f32(1)).astype(f32)
    return out, (v * aY2).astype(f32)


def variance_inputs(Hh, W, seed):
    """A variance plane for filter_inputs(Hh, W, .): values over six decades, zeros, values to 1e6, a NaN and a negative"""
    rng = np.random.default_rng(seed + 1000)
    v = (f32(10.0) ** rng.uniform(-6, 0, (Hh, W)).astype(f32)).astype(f32)
    v[rng.random((Hh, W)) < 0.1] = 0
    v[rng.random((Hh, W)) < 0.02] = f32(1e6)
    v.flat[v.size // 2] = f32(-3.0)
    v.flat[0] = np.nan
    if v.size > 5:
        v.flat[5] = f32(1e6); v.flat[3] = 0
    return v
