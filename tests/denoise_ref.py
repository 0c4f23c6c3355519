"""The denoiser's definition (INTEGRATION.md "Guides and denoising") restated in numpy float32, independent of the library: vectorised over
pixels, the 25 taps looped in the stated order (dy outer, dx inner).  Plus the test inputs of the filter tests and the counter sampler's
camera rays.  Shared by test_denoise_host.py (CPU: the restatement raises no floating-point exception) and test_gpu_denoise.py."""
import numpy as np

f32 = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)       # exact in binary


def _sq3(d):
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def atrous_ref(film, albedo, normal, depth, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.03, demodulate=True):
    """(H, W, 3) film, albedo, normal; (H, W) depth -> (H, W, 3) float32.  Every operation is one float32 operation, in the order written."""
    film = np.asarray(film, f32); normal = np.asarray(normal, f32); z = np.asarray(depth, f32)
    Hh, W = z.shape
    a = np.maximum(np.asarray(albedo, f32), f32(0.001)).astype(f32) if demodulate else np.ones_like(film)
    c = (film / a).astype(f32)
    sc, sn, sz = f32(sigma_color), f32(sigma_normal), f32(sigma_depth)
    kn = f32(1) / (sn * sn); kz = f32(1) / (sz * sz); sc2 = sc * sc
    one = f32(1)
    for i in range(iterations):
        s = 1 << i
        kc = f32(4.0 ** i) / sc2
        num = np.zeros_like(c); den = np.zeros((Hh, W), f32)
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
                w = (hh / (((one + (dc * kc).astype(f32)).astype(f32) * (one + (dn * kn).astype(f32)).astype(f32)).astype(f32)
                           * (one + (dz * kz).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                num[P] = (num[P] + (w[..., None] * c[Q]).astype(f32)).astype(f32)
                den[P] = (den[P] + w).astype(f32)
        c = (num / den[..., None]).astype(f32)
    return np.minimum(np.maximum((c * a).astype(f32), f32(0)), f32(1)).astype(f32)


def filter_inputs(Hh, W, seed):
    """A random film in [0, 1] and guides with flat regions, a normal edge, a depth edge, a depth ramp, miss regions (n = 0, z = 0), albedo
    with zeros and values below 0.001"""
    rng = np.random.default_rng(seed)
    film = rng.random((Hh, W, 3), dtype=f32)
    yy, xx = np.mgrid[0:Hh, 0:W]
    normal = np.zeros((Hh, W, 3), f32); normal[..., 2] = 1
    normal[:, W // 2:] = np.array([0.6, 0.0, 0.8], f32)                                  # a normal edge
    depth = np.full((Hh, W), 10.0, f32)
    depth[Hh // 3:, :] = f32(25.0)                                                         # a depth edge
    depth[2 * Hh // 3:, :] = (f32(25.0) + xx[2 * Hh // 3:, :].astype(f32) * f32(0.125)).astype(f32)   # a ramp
    albedo = np.where(((xx // 4 + yy // 4) % 2 == 0)[..., None], np.array([0.8, 0.7, 0.6], f32), np.array([0.2, 0.3, 0.9], f32)).astype(f32)
    miss = (yy < max(1, Hh // 8)) & (xx > W // 4)                                          # a miss band: n = 0, z = 0, albedo 1
    normal[miss] = 0; depth[miss] = 0; albedo[miss] = 1
    albedo[Hh // 2, :] = 0                                                                 # a row of zeros
    albedo[:, W // 3] = f32(0.0004)                                                        # a column below the 0.001 floor
    return film, albedo, normal, depth


def mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def rng_key(seed, x, y, s):
    k = mix32(np.uint32(seed) ^ np.full_like(x, 0x9E3779B9, dtype=np.uint32))
    k = mix32(k + x.astype(np.uint32)); k = mix32(k + y.astype(np.uint32)); k = mix32(k + np.uint32(s))
    return k


def rng_float(key, dim):
    return ((mix32(key + np.uint32((dim * 0x9E3779B9) & 0xffffffff)) >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def camera_rays(cam, W, Hh, seed, s, debug=False):
    """the camera ray of sample s of every pixel (row-major), as k_raygen forms it: dims 0 and 1 of the pixel's key (debug sampler: the centre)"""
    with np.errstate(over="ignore"):
        yy, xx = np.mgrid[0:Hh, 0:W]
        x = xx.ravel(); y = yy.ravel()
        key = rng_key(seed, x, y, s)
        u0 = np.full(x.shape, 0.5, f32) if debug else rng_float(key, 0)
        u1 = np.full(x.shape, 0.5, f32) if debug else rng_float(key, 1)
    fx = (x.astype(f32) + u0).astype(f32); fy = (y.astype(f32) + u1).astype(f32)
    pos, front, right, up = (np.array(getattr(cam, k), f32) for k in ("pos", "front", "right", "up"))
    a = ((fx / f32(cam.res_x)).astype(f32) - f32(0.5)).astype(f32); b = (f32(0.5) - (fy / f32(cam.res_y)).astype(f32)).astype(f32)
    d = ((front[None, :] + (right[None, :] * a[:, None]).astype(f32)).astype(f32) + (up[None, :] * b[:, None]).astype(f32)).astype(f32)
    ln = np.sqrt(_sq3(d)).astype(f32)
    d = (d / ln[:, None]).astype(f32)
    o = np.tile(pos, (d.shape[0], 1)).astype(f32)
    return o, d, np.full(len(d), 1e-3, f32), np.full(len(d), np.inf, f32)
