"""The records, points and widths the procedural-texture tests share (tests/test_procedural_host.py on the CPU, tests/test_gpu_procedural.py on the device)."""
import numpy as np

import jet_pbrt_amd as jp
import procedural_ref as R

f32 = np.float32
C_EVEN = (0.125, 0.5, 0.875)
C_ODD = (1.0, 0.25, 0.0)
SCALED = (2.0, 0.5, 0.0, 0.25, -0.5, 1.5, 0.25, -1.0, 0.0, 0.25, 3.0, 0.5)       # a general affine map, not singular
KINDS = [R.NOISE, R.FBM, R.TURBULENCE, R.MARBLE, R.CHECKER_AA]


def record(kind, space=R.WORLD, m=R.IDENTITY, octaves=0, gain=0.0, variation=0.0, antialias=0):
    """(the JpProcedural, the restatement's dict) of one record"""
    d = dict(kind=kind, space=space, m=m, octaves=octaves, gain=gain, variation=variation, antialias=antialias)
    return jp.procedural(kind, space, m, octaves, gain, variation, antialias), d


def records():
    """every kind in both spaces: identity map with the defaults, and a general map with its own octaves, gain and variation"""
    out = []
    for kind in KINDS:
        for space in (R.WORLD, R.UV):
            out.append(record(kind, space))
            out.append(record(kind, space, SCALED, octaves=3, gain=0.75, variation=2.5))
    out.append(record(R.FBM, antialias=-1))
    out.append(record(R.TURBULENCE, octaves=12, gain=1.0))
    return out


def points(n_random=192, seed=7):
    """lattice points, negative cells, |q| near 2^24, NaN / infinity, denormals and a random set: (p (n, 3), uv (n, 2))"""
    big = float(2 ** 24)
    below = float(np.nextafter(f32(big), f32(0)))
    p = [(0, 0, 0), (1, 2, 3), (-1, -2, -3), (-4, 7, -9), (255, -256, 1024), (0.5, 0.5, 0.5), (-0.5, -0.5, -0.5), (-0.25, -1.75, -3.125), (-1e-3, -1e-3, -1e-3),
         (big, 0, 0), (0, -big, 0), (below, below, below), (-below, 0.25, -below), (big / 2 + 0.5, 3, 3), (big / 32, big / 64, -big / 32), (2 * big, 1, 1),
         (np.nan, 0, 0), (0, np.nan, 0.5), (np.inf, 1, 1), (1, -np.inf, 1), (0.5, 0.5, np.inf), (1e30, -1e30, 1e30), (1e-40, -1e-40, 1e-45), (-0.0, 0.0, -0.0),
         (3.4e38, 3.4e38, -3.4e38), (0.3141, 0.6283, 0.9424), (1.5707964, 0.1, 0.1)]
    rng = np.random.default_rng(seed)
    p = np.concatenate([np.array(p, f32), rng.uniform(-6, 6, (n_random, 3)).astype(f32), rng.uniform(-300, 300, (n_random // 4, 3)).astype(f32)])
    uv = rng.uniform(-1.5, 2.5, (p.shape[0], 2)).astype(f32)
    uv[:8] = np.array([(0, 0), (1, 1), (-1, -2), (0.5, 0.5), (np.nan, 0), (0, np.inf), (1e30, 0), (-3, 4)], f32)
    return p, uv


def _width_landing_on(k, s):
    """a float32 width with float32(width * s) == k exactly (the footprint is fw = width * s, one rounded product)"""
    x = f32(k / s)
    for _ in range(64):
        fw = f32(x * s)
        if fw == k:
            return x
        x = np.nextafter(x, f32(0) if fw > k else f32(1e9))
    raise AssertionError("no float32 width lands on %r under s = %r" % (k, s))


def widths():
    """0, the fade boundaries k_i = 0.25 and 0.5 of octave 0 and of octaves 2, 5 and 11 (the last of the records above) with their float neighbours -- for the
    identity map (s = 1) and for SCALED (its own s) --, the checker's two thresholds, and hostile values"""
    w = [0.0, -1.0, np.nan, np.inf, 1e-45, 1e-30, 1e30, 0.01, 0.1, 0.3, 0.37, 0.7, 3.0, 100.0, 5000.0]
    for octave in (0, 2, 5, 11):
        for k in (0.25, 0.5):
            x = f32(k / 2 ** octave)
            w += [float(x), float(np.nextafter(x, f32(0))), float(np.nextafter(x, f32(1)))]
    # the same boundaries for the records under SCALED (s != 1, 3 octaves: first octave 0, last octave 2): a width whose product with s is the boundary exactly
    s = R.resolve(dict(kind=R.FBM, m=SCALED))["s"]
    for octave in (0, 2):
        for k in (0.25, 0.5):
            x = _width_landing_on(f32(k / 2 ** octave), s)
            w += [float(x), float(np.nextafter(x, f32(0))), float(np.nextafter(x, f32(1)))]
    for fy in (R.CHECKER_MIN, R.CHECKER_MAX):
        x = f32(fy / R.TEN_OVER_PI)
        w += [float(x), float(np.nextafter(x, f32(0))), float(np.nextafter(x, f32(1e9)))]
    return np.array(w, f32)


def grid(n=None, seed=3):
    """points x widths as flat arrays (p, uv, width); n: that many of them, drawn in a fixed order (None: all)"""
    p, uv = points()
    w = widths()
    P = np.repeat(p, w.shape[0], 0); U = np.repeat(uv, w.shape[0], 0); W = np.tile(w, p.shape[0])
    if n is None:
        return P, U, W
    idx = np.random.default_rng(seed).permutation(P.shape[0])[:n]
    idx[: min(n, 8)] = np.arange(min(n, 8)) * w.shape[0]                     # keep the first hostile points whatever n is
    return P[idx], U[idx], W[idx]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
