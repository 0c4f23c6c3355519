"""Procedural textures in numpy, restated from the text of INTEGRATION.md "Procedural textures" (not from the C code): the lattice hash, Perlin's improved noise,
the octave weights with their early exit, the five kinds and the side word.  Every float operation is one float32 operation in the order of the text."""
import numpy as np

f32 = np.float32
NONE, NOISE, FBM, TURBULENCE, MARBLE, CHECKER_AA = range(6)
WORLD, UV = 0, 1
SEED = 0x50524F43
LIMIT = f32(16777216.0)
TEN_OVER_PI = f32(3.1830988)
CHECKER_MIN = f32(0.03125)
CHECKER_MAX = f32(4096.0)
TAG_IMAGE = 0x80000000
TAG_COLOR = 0x40000000
M32 = np.uint64(0xFFFFFFFF)
IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def lattice_hash(ix, iy, iz):
    """jp_rng_key(SEED, ix, iy, iz) on integer arrays (wrapping as uint32)"""
    k = mix32(np.uint64(SEED ^ 0x9E3779B9))
    for c in (ix, iy, iz):
        k = mix32((k + (np.asarray(c, np.int64).astype(np.uint64) & M32)) & M32)
    return k


def in_range(x):
    with np.errstate(all="ignore"):
        return np.isfinite(x) & (x > -LIMIT) & (x < LIMIT)


def clamp01(x):
    with np.errstate(all="ignore"):
        return np.where(~(x > 0), f32(0), np.where(x > 1, f32(1), x)).astype(f32)


def grad(h, x, y, z):
    h = (h & np.uint64(15)).astype(np.int64)
    u = np.where(h < 8, x, y).astype(f32)
    v = np.where(h < 4, y, np.where((h == 12) | (h == 14), x, z)).astype(f32)
    return (np.where(h & 1, -u, u).astype(f32) + np.where(h & 2, -v, v).astype(f32)).astype(f32)


def fade(t):
    t = t.astype(f32)
    a = (((t * f32(6)).astype(f32) - f32(15)).astype(f32) * t).astype(f32)
    return ((((t * t).astype(f32) * t).astype(f32)) * (a + f32(10)).astype(f32)).astype(f32)


def lerp(a, b, w):
    return (a + (w * (b - a).astype(f32)).astype(f32)).astype(f32)


def noise(qx, qy, qz):
    qx, qy, qz = (np.asarray(a, f32) for a in (qx, qy, qz))
    ok = in_range(qx) & in_range(qy) & in_range(qz)
    sx, sy, sz = (np.where(ok, a, f32(0)).astype(f32) for a in (qx, qy, qz))
    fx, fy, fz = np.floor(sx), np.floor(sy), np.floor(sz)
    ix, iy, iz = fx.astype(np.int64), fy.astype(np.int64), fz.astype(np.int64)
    x, y, z = (sx - fx).astype(f32), (sy - fy).astype(f32), (sz - fz).astype(f32)
    x1, y1, z1 = (x - f32(1)).astype(f32), (y - f32(1)).astype(f32), (z - f32(1)).astype(f32)
    g = {}
    for dz, zz in ((0, z), (1, z1)):
        for dy, yy in ((0, y), (1, y1)):
            for dx, xx in ((0, x), (1, x1)):
                g[dx, dy, dz] = grad(lattice_hash(ix + dx, iy + dy, iz + dz), xx, yy, zz)
    u, v, w = fade(x), fade(y), fade(z)
    a = lerp(g[0, 0, 0], g[1, 0, 0], u); b = lerp(g[0, 1, 0], g[1, 1, 0], u); c = lerp(g[0, 0, 1], g[1, 0, 1], u); d = lerp(g[0, 1, 1], g[1, 1, 1], u)
    e = lerp(a, b, v); f = lerp(c, d, v)
    n = lerp(e, f, w)
    n = np.where(n < -1, f32(-1), np.where(n > 1, f32(1), n)).astype(f32)
    return np.where(ok, n, f32(0)).astype(f32)


def weight(k):
    with np.errstate(all="ignore"):
        return np.where(k <= f32(0.25), f32(1), np.where(k >= f32(0.5), f32(0), ((f32(0.5) - k).astype(f32) * f32(4)).astype(f32))).astype(f32)


def octaves_sum(q, fw, octaves, gain, turb):
    n = q.shape[0]
    s = np.zeros(n, f32); amp = f32(1); f = f32(1); k = fw.astype(f32).copy()
    alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(octaves):
            a = weight(k)
            alive &= a != 0
            nz = noise((f * q[:, 0]).astype(f32), (f * q[:, 1]).astype(f32), (f * q[:, 2]).astype(f32))
            if turb:
                term = (((a * amp).astype(f32) * np.abs(nz)).astype(f32) + (((f32(1) - a).astype(f32) * amp).astype(f32) * f32(0.2)).astype(f32)).astype(f32)
                tail = f32(amp * f32(0.2))
                s = np.where(alive, (s + term).astype(f32), (s + tail).astype(f32)).astype(f32)
            else:
                s = np.where(alive, (s + ((a * amp).astype(f32) * nz).astype(f32)).astype(f32), s).astype(f32)
            amp = f32(amp * gain); f = f32(f * f32(2)); k = (k * f32(2)).astype(f32)
    return s


def resolve(rec):
    """rec: dict(kind, space, m, octaves, gain, variation, antialias) -> the resolved record (defaults, norm, s)"""
    m = np.asarray(rec.get("m", IDENTITY), f32)
    octv = 1 if rec["kind"] == NOISE else (rec.get("octaves", 0) or 6)
    gain = f32(rec.get("gain", 0) or 0.5)
    var = f32(rec.get("variation", 0) or 1.0)
    acc = f32(0); amp = f32(1)
    for _ in range(octv):
        acc = f32(acc + amp); amp = f32(amp * gain)
    norm = f32(f32(1) / acc)
    best = f32(0)
    for k in range(3):
        n2 = f32(f32(f32(m[k] * m[k]) + f32(m[4 + k] * m[4 + k])) + f32(m[8 + k] * m[8 + k]))
        if n2 > best:
            best = n2
    s = f32(0) if rec.get("antialias", 0) < 0 else f32(np.sqrt(best))
    return dict(kind=rec["kind"], space=rec.get("space", WORLD), m=m, octaves=octv, gain=gain, variation=var, norm=norm, s=s)


def tri_integral(y):
    r = (y - (f32(2) * np.floor((y * f32(0.5)).astype(f32))).astype(f32)).astype(f32)
    return np.where(r < 1, r, (f32(2) - r).astype(f32)).astype(f32)


def square_mean(y, fy):
    h = (fy * f32(0.5)).astype(f32)
    m = ((tri_integral((y + h).astype(f32)) - tri_integral((y - h).astype(f32))).astype(f32) / fy).astype(f32)
    return np.where(m < -1, f32(-1), np.where(m > 1, f32(1), m)).astype(f32)


def byte(r):
    with np.errstate(all="ignore"):
        q = ((f32(255) * r).astype(f32) + f32(0.5)).astype(f32)
        return np.where(q > 0, np.where(q < 256, np.where(np.isfinite(q), q, 0).astype(np.int64), 255), 0).astype(np.uint32)


def word_of(c_even, c_odd, t):
    ce = np.asarray(c_even, f32); co = np.asarray(c_odd, f32)
    out = np.full(t.shape[0], TAG_IMAGE, np.uint32)
    with np.errstate(all="ignore"):
        for k in range(3):
            r = (ce[k] + (t * f32(co[k] - ce[k])).astype(f32)).astype(f32)
            out |= byte(r) << np.uint32(8 * k)
    return out


def fragile(rec, p, uv):
    """points of a CHECKER_AA record where the plain checker's parity hangs on the last bit of a sine: the product of the three sines is not 0 but within a factor
    2^20 of float32's underflow (see lookup)"""
    if rec["kind"] != CHECKER_AA:
        return np.zeros(np.asarray(p, f32).reshape(-1, 3).shape[0], bool)
    r = resolve(rec)
    p = np.asarray(p, f32).reshape(-1, 3); n = p.shape[0]
    uv = np.broadcast_to(np.asarray(uv, f32), (n, 2)); m = r["m"].astype(np.float64)
    x = np.stack([uv[:, 0], uv[:, 1], np.zeros(n, f32)], -1) if r["space"] == UV else p
    with np.errstate(all="ignore"):
        q = np.stack([m[4 * k] * x[:, 0] + m[4 * k + 1] * x[:, 1] + m[4 * k + 2] * x[:, 2] + m[4 * k + 3] for k in range(3)], -1)
        prod = np.abs(np.sin(10 * q[:, 0]) * np.sin(10 * q[:, 1]) * np.sin(10 * q[:, 2]))
        return np.isfinite(prod) & (prod > 0) & (prod < 2.0 ** -129)


def lookup(rec, c_even, c_odd, p, uv, width, texture=0):
    """-> (word (n,) uint32, t (n,) float32)"""
    r = resolve(rec)
    p = np.asarray(p, f32).reshape(-1, 3); n = p.shape[0]
    uv = np.broadcast_to(np.asarray(uv, f32), (n, 2)); width = np.broadcast_to(np.asarray(width, f32), (n,))
    m = r["m"]
    with np.errstate(all="ignore"):
        if r["space"] == UV:
            x = np.stack([uv[:, 0], uv[:, 1], np.zeros(n, f32)], -1).astype(f32)
        else:
            x = p
        q = np.stack([((((m[4 * k] * x[:, 0]).astype(f32) + (m[4 * k + 1] * x[:, 1]).astype(f32)).astype(f32) + (m[4 * k + 2] * x[:, 2]).astype(f32)).astype(f32) + m[4 * k + 3]).astype(f32)
                      for k in range(3)], -1)
        fw = (width * r["s"]).astype(f32)
        fw = np.where(fw > 0, fw, f32(0)).astype(f32)
        kind = r["kind"]
        if kind == CHECKER_AA:
            fy = (fw * TEN_OVER_PI).astype(f32)
            ok = in_range(q[:, 0]) & in_range(q[:, 1]) & in_range(q[:, 2])
            qs = np.where(ok[:, None], q, f32(0)).astype(f32)
            plain = ok & (fy <= CHECKER_MIN)
            # The plain checker is the one branch with a libm call: the library takes the host's sincosf, this restatement the float64 sine rounded to float32.
            # The two may differ in the last bit of a sine.  Only the SIGN of the float32 product is used; no float32 argument lies close enough to a multiple
            # of pi for a last bit to change a sine's sign, so the signs agree unless the product underflows (three sines of denormal size).  fragile() names
            # those points, and the bit-for-bit test leaves them out, so it does not depend on the libm build.
            s3 = [np.sin((f32(10) * qs[:, k]).astype(f32).astype(np.float64)).astype(f32) for k in range(3)]
            even = ~(((s3[0] * s3[1]).astype(f32) * s3[2]).astype(f32) < 0)
            fys = np.where(plain | ~(fy < CHECKER_MAX), f32(1), fy).astype(f32)
            ms = [square_mean((qs[:, k] * TEN_OVER_PI).astype(f32), fys) for k in range(3)]
            tf = ((f32(1) - ((ms[0] * ms[1]).astype(f32) * ms[2]).astype(f32)).astype(f32) * f32(0.5)).astype(f32)
            t = np.where(~ok | ~(fy < CHECKER_MAX), f32(0.5), tf).astype(f32)
            t = np.where(plain, np.where(even, f32(0), f32(1)), t).astype(f32)
            w = word_of(c_even, c_odd, t)
            w = np.where(plain, np.uint32(TAG_COLOR) | (np.uint32(2 * texture) + even.astype(np.uint32)), w).astype(np.uint32)
            return w, t
        if kind == NOISE:
            t = clamp01((f32(0.5) + (f32(0.5) * (weight(fw) * noise(q[:, 0], q[:, 1], q[:, 2])).astype(f32)).astype(f32)).astype(f32))
        elif kind == FBM:
            t = clamp01((f32(0.5) + (f32(0.5) * (r["norm"] * octaves_sum(q, fw, r["octaves"], r["gain"], False)).astype(f32)).astype(f32)).astype(f32))
        elif kind == TURBULENCE:
            t = clamp01((r["norm"] * octaves_sum(q, fw, r["octaves"], r["gain"], True)).astype(f32))
        else:
            s = (q[:, 1] + (r["variation"] * octaves_sum(q, fw, r["octaves"], r["gain"], False)).astype(f32)).astype(f32)
            d = (s - np.floor((s + f32(0.5)).astype(f32))).astype(f32)
            y = clamp01((f32(2) * np.abs(d)).astype(f32))
            t = ((y * y).astype(f32) * (f32(3) - (f32(2) * y).astype(f32)).astype(f32)).astype(f32)
    return word_of(c_even, c_odd, t), t
