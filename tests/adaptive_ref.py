"""The adaptive sampling loop (INTEGRATION.md "Adaptive sampling") restated in numpy float32, independent of the library: vectorised over the pixels of an
unsharded image, every operation one float32 operation in the order include/jp_adaptive.h writes it.  Also the synthetic sample sets the tests share: pixels
whose samples are constant pass the first test, pixels that alternate between two values never pass, so the surviving set is chosen pixel by pixel.
Shared by test_adaptive_host.py (CPU) and test_gpu_adaptive.py."""
import numpy as np

from variance_ref import _lum, clamp_samples_ref

f32 = np.float32
H, W = 24, 40                                                                # 960 pixels: not a multiple of 256
SURVIVORS = (0, 1, 255, 256, 257, 959, 960)


def passes_ref(mean, m2, n, threshold, floor):
    """jp_adapt_pass per pixel; n: int array of the pixels' own counts (>= 2)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.where(mean > f32(floor), mean, f32(floor)).astype(f32)
        t = (f32(threshold) * m).astype(f32)
        tt = (t * t).astype(f32)
        v = ((m2 / (n - 1).astype(f32)).astype(f32) / n.astype(f32)).astype(f32)
        return ~np.isfinite(v) | ~np.isfinite(tt) | (v <= tt)


def fails_nearby(fail):
    """(H, W) bool -> does a pixel of the 3 x 3 neighbourhood, clipped to the image, fail"""
    h, w = fail.shape
    pad = np.zeros((h + 2, w + 2), bool); pad[1:-1, 1:-1] = fail
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def adaptive_ref(samples, height, width, min_spp, step_spp, threshold, floor=0.0, dilate=1, sample_clamp=0.0, hdr=0, trace=None):
    """(max_spp, height * width, 3) float32 samples -> (film (H, W, 3), counts (H, W) int32, variance (H, W)); trace: a list that receives the active count after
    every test"""
    s = np.asarray(samples, f32)
    max_spp, npix = s.shape[:2]
    assert npix == height * width and 2 <= min_spp <= max_spp and step_spp >= 1
    if sample_clamp > 0:
        s = clamp_samples_ref(sample_clamp, s)
    floor = f32(floor) if floor > 0 else f32(1e-3)
    total = np.zeros((npix, 3), f32); mean = np.zeros(npix, f32); m2 = np.zeros(npix, f32)
    n = np.zeros(npix, np.int32); active = np.ones(npix, bool)
    n_cur, ns = 0, min_spp
    with np.errstate(invalid="ignore", over="ignore"):
        while active.any():
            a = np.nonzero(active)[0]
            for k in range(n_cur, n_cur + ns):
                l = s[k, a]
                total[a] = (total[a] + l).astype(f32)
                y = _lum(l).astype(f32)
                y = np.where(np.isfinite(y), y, f32(0)).astype(f32)
                d = (y - mean[a]).astype(f32)
                mean[a] = (mean[a] + (d / f32(k + 1)).astype(f32)).astype(f32)
                m2[a] = (m2[a] + (d * (y - mean[a]).astype(f32)).astype(f32)).astype(f32)
            n[a] = n_cur + ns
            n_cur += ns
            if n_cur >= max_spp:
                break
            fail = ~passes_ref(mean, m2, n, threshold, floor)
            if dilate:
                fail = fails_nearby(fail.reshape(height, width)).reshape(-1)
            active = active & fail
            if trace is not None:
                trace.append(int(active.sum()))
            ns = min(step_spp, max_spp - n_cur)
        film = (total / n.astype(f32)[:, None]).astype(f32)
        film = np.where(film > 0, film, f32(0)).astype(f32)                  # (a NaN compares false: 0, as the header's v > 0 ? ... : 0)
        if not hdr:
            film = np.where(film < 1, film, f32(1)).astype(f32)
        var = ((m2 / (n - 1).astype(f32)).astype(f32) / n.astype(f32)).astype(f32)
    return film.reshape(height, width, 3), n.reshape(height, width), var.reshape(height, width)


def survivor_pixels(k, seed=0):
    """k pixel indices of the H x W image: none, the bottom-right corner alone, or a seeded choice (all of them for k = 960)"""
    if k == 1:
        return np.array([H * W - 1])
    return np.sort(np.random.default_rng(seed + k).permutation(H * W)[:k])


def synthetic_samples(noisy, max_spp, seed=0, hostile=False):
    """(max_spp, H * W, 3) float32: a pixel of `noisy` alternates between two colours (relative error of the mean about 1 / sqrt(n): it fails any threshold
    below 0.1 up to 64 samples), every other pixel repeats one colour (variance exactly 0: it passes).  hostile: a NaN and an infinite channel in noisy
    pixels' later samples, and a constant pixel brighter than 1"""
    rng = np.random.default_rng(seed)
    npix = H * W
    base = (rng.random((npix, 3), dtype=f32) * f32(0.75) + f32(0.125)).astype(f32)
    base = (np.round(base * 64) / 64).astype(f32)                            # a few mantissa bits: the running mean of a constant pixel is exact, m2 stays 0
    s = np.repeat(base[None], max_spp, 0).copy()
    noisy = np.asarray(noisy, np.int64)
    if noisy.size:
        odd = (np.arange(max_spp) % 2 == 1)
        hi = (base[noisy] * f32(2.5)).astype(f32); lo = (base[noisy] * f32(0.25)).astype(f32)
        s[:, noisy] = np.where(odd[:, None, None], hi[None], lo[None])
    if hostile:
        quiet = np.setdiff1d(np.arange(npix), noisy)
        if noisy.size:
            s[max_spp - 1, noisy[0], 1] = np.nan
            s[min(max_spp - 1, 9), noisy[-1], 2] = np.inf
        if quiet.size:
            s[:, quiet[0]] = np.array([3.0, 0.5, 2.0], f32)
    return s
