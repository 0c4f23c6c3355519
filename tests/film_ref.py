"""The film's definitions (INTEGRATION.md "Film") restated in numpy, independent of the library: the fp32 sample clamp, the luminance histogram by
integer bit operations, the exposure in float64, the four curves in np.float32 operation by operation, the byte lookup from the gamma thresholds, and the
HDR last step of the denoiser on top of denoise_ref.  Plus the adversarial vector the host and GPU tests share.
Shared by test_film_host.py (CPU) and test_gpu_film.py."""
import math

import numpy as np

import denoise_ref as DR

f32 = np.float32
BINS = 256
CLAMP, REINHARD, ACES, HABLE = 0, 1, 2, 3
MANUAL, AUTO = 0, 1
DEFAULTS = dict(key=0.18, white=4.0, pct_low=0.05, pct_high=0.95)


def _finite(x):
    return (np.asarray(x, f32).view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)


def sample_clamp(c, rgb):
    """(n, 3) float32 radiances -> (n, 3): any channel not finite -> 0; m = max(max(r, g), b) > c -> l * (c / m); else l"""
    a = np.ascontiguousarray(rgb, f32).reshape(-1, 3)
    out = a.copy()
    if not c > 0:
        return out
    c = f32(c)
    fin = _finite(a).all(axis=1)
    with np.errstate(all="ignore"):
        m = np.maximum(np.maximum(a[:, 0], a[:, 1]), a[:, 2]).astype(f32)
        over = fin & (m > c)
        k = (c / m[over]).astype(f32)
        out[over] = (a[over] * k[:, None]).astype(f32)
    out[~fin] = 0
    return out


def luminance(film):
    a = np.ascontiguousarray(film, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (((f32(0.2126) * a[:, 0]).astype(f32) + (f32(0.7152) * a[:, 1]).astype(f32)).astype(f32) + (f32(0.0722) * a[:, 2]).astype(f32)).astype(f32)


def histogram(film):
    """BINS + 1 uint32 counts of a (..., 3) film; the last one: the excluded pixels"""
    Y = luminance(film)
    with np.errstate(invalid="ignore"):
        ok = (Y > 0) & _finite(Y)
    k = (Y[ok].view(np.uint32) >> np.uint32(21)).astype(np.int64) - 380
    k = np.clip(k, 0, BINS - 1)
    h = np.zeros(BINS + 1, np.uint32)
    h[:BINS] = np.bincount(k, minlength=BINS).astype(np.uint32)
    h[BINS] = np.count_nonzero(~ok)
    return h


def _resolved(tm):
    """a dict of a JpToneMap-like object (fields curve, exposure_mode, ev, key, white, pct_low, pct_high) with the defaults filled in, every value rounded to fp32"""
    d = dict(curve=int(tm.curve), exposure_mode=int(tm.exposure_mode), ev=f32(tm.ev))
    for name, dflt in DEFAULTS.items():
        v = f32(getattr(tm, name))
        d[name] = f32(dflt) if v == 0 else v
    return d


def exposure(tm, hist):
    """the exposure scale (a float32) in float64 arithmetic"""
    t = _resolved(tm)
    ev = float(t["ev"])
    if t["exposure_mode"] == MANUAL:
        return f32(2.0 ** ev)
    h = np.asarray(hist[:BINS], np.float64)
    N = 0.0
    for v in h:
        N += v
    if not N > 0:
        return f32(1.0)
    lo, hi = float(t["pct_low"]) * N, float(t["pct_high"]) * N
    cum = sw = sl = 0.0
    for k in range(BINS):
        a, b = cum, cum + h[k]
        cum = b
        c = min(b, hi) - max(a, lo)
        if not c > 0:
            continue
        centre = (1.125 + 0.25 * (k & 3)) * 2.0 ** ((k >> 2) - 32)
        sw += c
        sl += c * math.log2(centre)
    if not sw > 0:
        return f32(1.0)
    return f32(float(t["key"]) / 2.0 ** (sl / sw) * 2.0 ** ev)


def _hable_h(x):
    x = np.asarray(x, f32)
    num = ((x * ((f32(0.15) * x).astype(f32) + f32(0.05)).astype(f32)).astype(f32) + f32(0.004)).astype(f32)
    den = ((x * ((f32(0.15) * x).astype(f32) + f32(0.5)).astype(f32)).astype(f32) + f32(0.06)).astype(f32)
    return ((num / den).astype(f32) - f32(0.02) / f32(0.3)).astype(f32)


def curve_values(tm, scale, x):
    """y in [0, 1] (float32, the shape of x) of the display transform under `scale`"""
    t = _resolved(tm)
    x = np.ascontiguousarray(x, f32)
    one = f32(1)
    with np.errstate(all="ignore"):
        tt = (x * f32(scale)).astype(f32)
        v = np.where(tt > 0, np.minimum(tt, f32(1e9)), f32(0)).astype(f32)
        if t["curve"] == REINHARD:
            w2 = t["white"] * t["white"]
            y = ((v * (one + (v / w2).astype(f32)).astype(f32)).astype(f32) / (one + v).astype(f32)).astype(f32)
        elif t["curve"] == ACES:
            num = (v * ((f32(2.51) * v).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
            den = ((v * ((f32(2.43) * v).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
            y = (num / den).astype(f32)
        elif t["curve"] == HABLE:
            y = (_hable_h((f32(2) * v).astype(f32)) / _hable_h(f32(11.2))).astype(f32)
        else:
            y = v
        return np.where(y < 0, f32(0), np.where(y > 1, f32(1), y)).astype(f32)


def gamma_bytes(thr255, y):
    """the number of thresholds <= y (uint8, the shape of y)"""
    return np.searchsorted(np.asarray(thr255, f32), np.asarray(y, f32), side="right").astype(np.uint8)


def atrous_hdr_ref(film, albedo, normal, depth, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.03, demodulate=True, shift=16):
    """The filter with max(c_n * a, 0) as its last step.  denoise_ref.atrous_ref ends with Clamp01; its arithmetic is exactly homogeneous under a power of
    two -- film and sigma_color scaled by 2^-shift scale c, num and the result by 2^-shift and leave every weight as it is (dc * kc is unchanged), as long
    as nothing leaves the normal range -- so the unclamped result is the clamped one of the scaled problem, scaled back, provided that one stayed below 1."""
    s = f32(2.0 ** -shift)
    out = DR.atrous_ref((np.asarray(film, f32) * s).astype(f32), albedo, normal, depth, iterations, f32(sigma_color) * s, sigma_normal, sigma_depth, demodulate)
    assert out.max() < 1, "atrous_hdr_ref: the scaled problem reached the upper clamp; raise shift"
    return (out * f32(2.0 ** shift)).astype(f32)


def adversarial_values():
    """0, -0, denormals, negatives, NaN, +-Inf, 1e9f and its neighbours, every power of two from 2^-40 to 2^40 and the fp32 value just below each, and 4096
    log-uniform random values: a float32 vector whose length is a multiple of 3"""
    special = np.array([0.0, -0.0, 1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.0, -0.5, -1e9, np.nan, np.inf, -np.inf, 0.18, 0.5, 1.0, 2.0, 4.0, 16.0, 3.4028235e38], f32)
    e9 = np.array([1e9], f32)
    near = np.concatenate([np.nextafter(e9, f32(0)), e9, np.nextafter(e9, f32(np.inf))]).astype(f32)
    p2 = (2.0 ** np.arange(-40, 41, dtype=np.float64)).astype(f32)
    below = np.nextafter(p2, f32(0)).astype(f32)
    rng = np.random.default_rng(20)
    rnd = (2.0 ** rng.uniform(-36.0, 36.0, 4096)).astype(f32)
    v = np.concatenate([special, near, p2, below, rnd]).astype(f32)
    pad = (-len(v)) % 3
    return np.concatenate([v, np.zeros(pad, f32)]).astype(f32)
