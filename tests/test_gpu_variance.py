"""Variance on the MI355X: the moments against their numpy restatement (exact), the variance-guided filter against its restatement (exact), the plumbing of
jp_render_variance through every schedule, that the plane is the variance of the film (against the spread of independently seeded films), that the filter
denoises, errors, and the host path."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import variance_ref as V

pytestmark = pytest.mark.gpu
f32 = np.float32
W = Hh = 64
IMG = np.random.default_rng(3).integers(0, 256, (23, 37, 3), dtype=np.uint8)      # the image of test_gpu_denoise.py's textured scene


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _l2(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum(-1)).mean())


def _lum64(film):
    f = film.astype(np.float64)
    return 0.2126 * f[..., 0] + 0.7152 * f[..., 1] + 0.0722 * f[..., 2]


# ---- 1. probe exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [0.0, 2.5])
def test_probe_equals_the_restatement(clamp):
    ctx = jp.Context(0)                                                       # a fresh context: no scene uploaded
    try:
        n, spp = 4096, 16
        rng = np.random.default_rng(5)
        s = (rng.random((spp, n, 3), dtype=f32) * (f32(10.0) ** rng.integers(-3, 3, (1, n, 1)).astype(f32))).astype(f32)
        s[:, 0] = f32(0.25); s[:, 1] = f32(0.5); s[7, 1] = f32(1e6); s[15, 2, 1] = np.nan; s[0, 3, 2] = np.inf; s[:, 4] = 0
        film = jp.film(0, clamp) if clamp > 0 else None
        want, _ = V.moments_ref(s, clamp)
        assert np.array_equal(_bits(jp.variance_samples(film, s)), _bits(want))
        for batch in (16, 5, 1):
            got = ctx.variance_probe(s, batch, film)
            bad = int((_bits(got) != _bits(want)).sum())
            if bad:
                print("probe batch %d clamp %g: %d pixels differ, max |d| %.3e" % (batch, clamp, bad, np.abs(got - want).max()))
            assert np.array_equal(_bits(got), _bits(want)), batch
        assert want[0] == 0 and want[4] == 0 and np.isfinite(want).all()
        assert ctx.lib.jp_variance_probe(ctx.h, None, 1, 1, n, s.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p)) == -1
        assert ctx.lib.jp_variance_probe(ctx.h, None, spp, 0, n, s.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p)) == -1
    finally:
        ctx.close()


# ---- 2. filter exact --------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 7), (67, 129), (200, 333)]                              # (H, W)
SIGMAS = [(2.0, 0.3, 0.1), (0.5, 0.1, 0.02)]


@pytest.mark.parametrize("size", SIZES)
def test_filter_bit_exact_against_numpy(size):
    ctx = jp.Context(0)
    try:
        h, w = size
        film, albedo, normal, depth = V.filter_inputs(h, w, 7)
        var = V.variance_inputs(h, w, 7)
        for hdr in (0, 1):
            ctx.set_film(hdr) if hdr else ctx.set_film(None)
            for it in range(1, 7):
                for demod in (True, False):
                    for sg in SIGMAS:
                        with np.errstate(over="raise", invalid="raise", divide="raise"):
                            want, want_v = V.atrous_v_ref(film, albedo, normal, depth, var, it, *sg, demodulate=demod, hdr=bool(hdr))
                        got, got_v = ctx.denoise_variance(film, albedo, normal, depth, var, iterations=it, sigma_color=sg[0], sigma_normal=sg[1], sigma_depth=sg[2],
                                                          demodulate=1 if demod else -1)
                        bad = int((got != want).any(-1).sum()); badv = int((_bits(got_v) != _bits(want_v)).sum())
                        if bad or badv:
                            print("filter %dx%d hdr %d it %d demod %s sigma %s: %d pixels differ (max |d| %.3e), %d variances (max |d| %.3e)"
                                  % (w, h, hdr, it, demod, sg, bad, np.abs(got - want).max(), badv, np.abs(got_v - want_v).max()))
                        assert np.array_equal(_bits(got), _bits(want)), (size, hdr, it, demod, sg)
                        assert np.array_equal(_bits(got_v), _bits(want_v)), (size, hdr, it, demod, sg)
        ctx.set_film(None)
        # the defaults: 5 iterations, sigma (8.0, 0.1, 0.03), demodulation on; variance_out may be NULL
        got, none = ctx.denoise_variance(film, albedo, normal, depth, var, want_variance=False)
        assert none is None and np.array_equal(_bits(got), _bits(V.atrous_v_ref(film, albedo, normal, depth, var)[0]))
        i = ctx.variance_info()
        assert i.iterations == 5 and (i.sigma_color, i.sigma_normal, i.sigma_depth) == (f32(8.0), f32(0.1), f32(0.03)) and i.demodulated == 1 and i.denoise_ms > 0
        assert i.variance_last_render == 0
    finally:
        ctx.close()


# ---- 3. plumbing --------------------------------------------------------------------------------------------------------------
def test_render_variance_film_schedules_shards_and_side_effects(gpu_ctx):
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=False)
    gpu_ctx.upload(be.flatten())
    rp = jp.render_params(W, Hh, 8, 5, 1234)
    film0 = gpu_ctx.render(rp); c0 = gpu_ctx.counters()
    assert gpu_ctx.variance_info().variance_last_render == 0
    alb, nrm, dep = gpu_ctx.render_guides(rp, 4)
    den0 = gpu_ctx.denoise(film0, alb, nrm, dep)
    film, var = gpu_ctx.render_variance(rp)
    b0 = jp.device_bytes_in_use()
    i = gpu_ctx.variance_info()
    assert i.variance_last_render == 1 and i.moment_bytes_device >= 8 * W * Hh
    assert np.array_equal(_bits(film), _bits(film0))
    assert var.shape == (Hh, W) and np.isfinite(var).all() and (var >= 0).all() and (var > 0).mean() > 0.5
    print("cornell 64x64 8 spp: variance mean %.3e max %.3e, zero in %.1f %% of the pixels" % (var.mean(), var.max(), 100 * (var == 0).mean()))
    _, again = gpu_ctx.render_variance(rp, want_film=False)
    assert np.array_equal(_bits(again), _bits(var))
    assert jp.device_bytes_in_use() == b0                                     # the moments live while a variance render runs: a second one leaves nothing behind
    try:
        for kw in (dict(lanes=1), dict(max_slots=4096), dict(blocks_per_cu=4), dict(fused=1), dict(lanes=3), dict(lanes=2, max_slots=4096)):
            gpu_ctx.set_options()                                             # (set_options changes fields of the options in force: back to the defaults first)
            gpu_ctx.set_options(**kw)
            f, v = gpu_ctx.render_variance(rp)
            if "fused" in kw:
                assert gpu_ctx.build_info().fused_last_render == 1
            if kw.get("lanes", 1) > 1:
                assert gpu_ctx.build_info().lanes_last_render == kw["lanes"]
            assert np.array_equal(_bits(f), _bits(film0)), kw
            assert np.array_equal(_bits(v), _bits(var)), kw
            assert np.array_equal(_bits(gpu_ctx.render(rp)), _bits(film0)), kw
    finally:
        gpu_ctx.set_options()
    gpu_ctx.render(rp)
    assert gpu_ctx.variance_info().moment_bytes_device == 0
    # band shards: disjoint, and they sum to the whole
    parts = [gpu_ctx.render_variance(jp.render_params(W, Hh, 8, 5, 1234, band_rows=20, shard_index=k, shard_count=2)) for k in range(2)]
    assert np.array_equal(_bits((parts[0][1] + parts[1][1]).astype(f32)), _bits(var)) and ((parts[0][1] != 0) & (parts[1][1] != 0)).sum() == 0
    assert np.array_equal(_bits((parts[0][0] + parts[1][0]).astype(f32)), _bits(film0))
    rows = (np.arange(Hh) // 20) % 2 == 0
    assert (parts[0][1][~rows] == 0).all() and (parts[1][1][rows] == 0).all()
    # the debug sampler: every sample of a pixel is the same -> exactly 0
    fd, vd = gpu_ctx.render_variance(jp.render_params(W, Hh, 8, 5, 1234, sampler_mode=jp.JP_SAMPLER_DEBUG))
    assert (vd == 0).all() and fd.mean() > 0.01
    # a film state: the film of jp_render under that state, and a variance that the sample clamp lowers
    try:
        gpu_ctx.set_film(1, 0.0)
        fh, vh = gpu_ctx.render_variance(rp)
        assert np.array_equal(_bits(fh), _bits(gpu_ctx.render(rp))) and np.array_equal(_bits(vh), _bits(var)) and gpu_ctx.film_info().hdr_last_render == 1
        gpu_ctx.set_film(1, 0.5)
        fc, vc = gpu_ctx.render_variance(rp)
        assert np.array_equal(_bits(fc), _bits(gpu_ctx.render(rp))) and vc.sum() < var.sum()
    finally:
        gpu_ctx.set_film(None)
    # Whitted delivers one too
    rw = jp.render_params(W, Hh, 8, 5, 1234, integrator=jp.JP_INTEGRATOR_WHITTED)
    fw, vw = gpu_ctx.render_variance(rw)
    assert np.array_equal(_bits(fw), _bits(gpu_ctx.render(rw))) and np.isfinite(vw).all() and (vw > 0).any()
    # ... and the render and the filter are what they were
    film1 = gpu_ctx.render(rp); c1 = gpu_ctx.counters()
    assert np.array_equal(_bits(film1), _bits(film0)) and gpu_ctx.variance_info().variance_last_render == 0
    for k in ("samples", "closest_rays", "closest_hits", "shadow_rays", "shadow_occluded"):
        assert getattr(c0, k) == getattr(c1, k), k
    assert np.array_equal(_bits(gpu_ctx.denoise(film1, alb, nrm, dep)), _bits(den0))
    # everything on the device between the stages = the stages one by one
    f, b8, a2, n2, z2, v2 = gpu_ctx.render_denoised_variance(rp, 4)
    want, _ = gpu_ctx.denoise_variance(film0, alb, nrm, dep, var)
    assert np.array_equal(_bits(f), _bits(want)) and np.array_equal(_bits(v2), _bits(var)) and np.array_equal(a2, alb) and np.array_equal(n2, nrm) and np.array_equal(z2, dep)
    thr = np.zeros(255, f32); assert gpu_ctx.lib.jp_gamma_thresholds(thr.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(b8, np.searchsorted(thr, want.ravel(), side="right").astype(np.uint8).reshape(Hh, W, 3))
    f, _, _, _, _, v2 = gpu_ctx.render_denoised_variance(rp, 4, denoise=False, want_bytes=False)
    assert np.array_equal(_bits(f), _bits(film0)) and np.array_equal(_bits(v2), _bits(var))


# ---- 4. it is the variance ------------------------------------------------------------------------------------------------------
def test_the_plane_is_the_variance_of_the_film(gpu_ctx):
    """256 independently seeded 4-spp films of the Lambert Cornell box (hdr: nothing clipped): S2_p, the per-pixel sample variance of their luminances, is the
    yardstick -- the films are pinned to the oracle.  Seeds in groups of 8; R_g = sum_p mean_g(reported variance) / sum_p S2_p with the denominator from all seeds.
    Asserted: |mean(R_g) - 1| <= 4 std(R_g) / sqrt(groups), and that standard error <= 0.05 (a missing Bessel correction is off by 25 %, a missing / spp by 4x).
    Seeds 1 .. 256, not 1 .. 64: sum_p S2_p is dominated by the few pixels on the lamp's edge (the largest holds 5 % of it), it is common to every group, and the
    spread between groups does not see its error.  With seeds 1 .. 64 the statistic is 0.9443 with a standard error of 0.0091 (it misses 4 standard errors), with
    1 .. 128 0.9468 / 0.0097, with 1 .. 256 0.9767 / 0.0072 -- and the textbook unbiased estimate computed in float64 from the oracle's per-sample luminances gives
    the same three pairs to four digits, so the miss at 64 seeds is the statistic's, not the kernel's."""
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=True)
    gpu_ctx.upload(be.flatten())
    n_seeds = 256
    try:
        gpu_ctx.set_film(1, 0.0)
        films, planes = zip(*[gpu_ctx.render_variance(jp.render_params(W, Hh, 4, 5, seed)) for seed in range(1, n_seeds + 1)])
    finally:
        gpu_ctx.set_film(None)
    Y = np.stack([_lum64(f) for f in films]); Vr = np.stack(planes).astype(np.float64)
    S2 = Y.var(axis=0, ddof=1)
    R = np.array([Vr[g * 8:(g + 1) * 8].mean(axis=0).sum() / S2.sum() for g in range(n_seeds // 8)])
    se = R.std(ddof=1) / np.sqrt(len(R))
    print("variance calibration, %d seeds: mean(R_g) %.4f, standard error %.4f, R_g %s" % (n_seeds, R.mean(), se, np.round(R, 4)))
    assert se <= 0.05
    assert abs(R.mean() - 1) <= 4 * se


# ---- 5. it denoises ---------------------------------------------------------------------------------------------------------------
def _denoise_case(ctx, name):
    w = h = 256
    ref = ctx.render(jp.render_params(w, h, 4096, 5, 99))
    rp = jp.render_params(w, h, 16, 5, 1234)
    noisy, var = ctx.render_variance(rp)
    alb, nrm, dep = ctx.render_guides(rp, 8)
    den_v, _ = ctx.denoise_variance(noisy, alb, nrm, dep, var)
    den = ctx.denoise(noisy, alb, nrm, dep)
    en, ev, ed = _l2(noisy, ref), _l2(den_v, ref), _l2(den, ref)
    print("%s 256x256 16 spp: meanL2 noisy %.5f, variance-guided %.5f (ratio %.3f), jp_denoise %.5f (ratio %.3f)" % (name, en, ev, ev / en, ed, ed / en))
    assert ev < en


def test_denoise_variance_reduces_error_cornell(gpu_ctx):
    be = scenes.build_cornell(scenes.HostBackend("c"), 256, 256, lambert_only=False)
    gpu_ctx.upload(be.flatten())
    _denoise_case(gpu_ctx, "cornell")


def test_denoise_variance_reduces_error_textured(gpu_ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("t"), 256, 256, back=lambda b: b.texture_image(IMG), floor=lambda b: b.texture_image(IMG[::-1].copy()))
    gpu_ctx.upload(be.flatten(), be.flatten_textures())
    _denoise_case(gpu_ctx, "textured cornell")


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(gpu_ctx):
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=True)
    gpu_ctx.upload(be.flatten())
    lib, hnd = gpu_ctx.lib, gpu_ctx.h
    film, albedo, normal, depth = V.filter_inputs(Hh, W, 2)
    var = V.variance_inputs(Hh, W, 2)
    out = np.zeros_like(film); vout = np.zeros_like(var)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def dn(dp, f=film, a=albedo, n=normal, z=depth, v=var, o=out, vo=vout):
        return lib.jp_denoise_variance(hnd, C.byref(dp), p(f), p(a), p(n), p(z), p(v), p(o), p(vo))
    INV = -1
    ok = jp.denoise_params(W, Hh)
    assert dn(ok, f=None) == INV and dn(ok, o=None) == INV and dn(ok, v=None) == INV and dn(ok, n=None) == INV
    assert b"jp_denoise_variance" in lib.jp_last_error() and b"null buffer" in lib.jp_last_error()
    assert dn(ok, a=None) == INV and dn(jp.denoise_params(W, Hh, demodulate=-1), a=None) == 0 and dn(ok, vo=None) == 0
    big = np.zeros(4 * var.size, f32)
    assert lib.jp_denoise_variance(hnd, C.byref(ok), p(film), p(albedo), p(normal), p(depth), p(big[var.size // 2:]), p(big), p(vout)) == INV   # out overlaps the variance
    assert b"overlaps" in lib.jp_last_error()
    assert dn(ok, o=film) == INV and dn(ok, vo=var) == INV and dn(ok, vo=depth) == INV
    assert lib.jp_denoise_variance(hnd, C.byref(ok), p(film), p(albedo), p(normal), p(depth), p(var), p(big), p(big[var.size:])) == INV          # variance_out inside out
    short = jp.denoise_params(W, Hh); short.struct_bytes = 12
    assert dn(short) == INV and b"struct_bytes" in lib.jp_last_error()
    assert dn(jp.denoise_params(W, Hh, iterations=7)) == INV and dn(jp.denoise_params(W, Hh, sigma_color=float("nan"))) == INV and dn(jp.denoise_params(0, Hh)) == INV
    # the render: spp = 1, null buffers
    rp1 = jp.render_params(W, Hh, 1)
    f = np.zeros((Hh, W, 3), f32); v = np.zeros((Hh, W), f32)
    assert lib.jp_render_variance(hnd, C.byref(rp1), p(f), p(v)) == INV
    assert b"jp_render_variance" in lib.jp_last_error() and b"spp" in lib.jp_last_error()
    rp = jp.render_params(W, Hh, 4)
    assert lib.jp_render_variance(hnd, C.byref(rp), None, None) == INV and lib.jp_render_variance(hnd, None, p(f), p(v)) == INV
    assert lib.jp_render_variance_device(hnd, C.byref(rp), None, None, 1) == INV
    assert lib.jp_render_denoised_variance(hnd, C.byref(rp1), 4, C.byref(ok), p(f), None, None, None, None, p(v)) == INV
    info = jp.JpVarianceInfo(); info.struct_bytes = 2
    assert lib.jp_get_variance_info(hnd, C.byref(info)) == INV and lib.jp_get_variance_info(hnd, None) == INV
    # ... and everything still works
    assert lib.jp_render_variance(hnd, C.byref(rp), None, p(v)) == 0 and (v > 0).any() and gpu_ctx.variance_info().variance_last_render == 1
    film4 = gpu_ctx.render(rp)
    assert gpu_ctx.variance_info().variance_last_render == 0
    assert lib.jp_render_variance(hnd, C.byref(rp), p(f), None) == 0 and np.array_equal(_bits(f), _bits(film4))
    got, got_v = gpu_ctx.denoise_variance(film, albedo, normal, depth, var, iterations=1)
    want, want_v = V.atrous_v_ref(film, albedo, normal, depth, var, 1)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_v), _bits(want_v))


# ---- 7. host path = C ABI path --------------------------------------------------------------------------------------------------------
def _host_variance(be, w, h, spp, seed, variance, guide_spp, denoise, hdr=0):
    film = np.zeros((h, w, 3), f32); var = np.zeros((h, w), f32)
    alb = np.zeros((h, w, 3), f32); nrm = np.zeros((h, w, 3), f32); dep = np.zeros((h, w), f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = jp.host_lib().jp_host_render_variance(be.h, w, h, spp, 5, seed, 0, variance, guide_spp, denoise, hdr, p(film), p(var), p(alb), p(nrm), p(dep))
    assert st == 0, st
    return film, var, alb, nrm, dep


def test_host_film_requests_equal_the_c_abi_calls(gpu_ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("t"), W, Hh, back=lambda b: b.texture_image(IMG))
    gpu_ctx.upload(be.flatten(), be.flatten_textures())
    rp = jp.render_params(W, Hh, 8, 5, 4321)
    noisy, var = gpu_ctx.render_variance(rp)
    assert np.array_equal(_bits(noisy), _bits(gpu_ctx.render(rp)))
    alb, nrm, dep = gpu_ctx.render_guides(rp, 8)
    den, _ = gpu_ctx.denoise_variance(noisy, alb, nrm, dep, var)
    assert not np.array_equal(den, noisy) and not np.array_equal(den, gpu_ctx.denoise(noisy, alb, nrm, dep))
    # FFilm::RequestVariance alone: the untouched film and the plane
    f, v, _, _, _ = _host_variance(be, W, Hh, 8, 4321, 1, 0, 0)
    assert np.array_equal(_bits(f), _bits(noisy)) and np.array_equal(_bits(v), _bits(var))
    # ... next to RequestGuides
    f, v, a, n, z = _host_variance(be, W, Hh, 8, 4321, 1, 8, 0)
    assert np.array_equal(_bits(f), _bits(noisy)) and np.array_equal(_bits(v), _bits(var)) and np.array_equal(a, alb) and np.array_equal(n, nrm) and np.array_equal(z, dep)
    # FFilm::RequestDenoise with FDenoiseOptions::varianceGuided
    f, v, a, n, z = _host_variance(be, W, Hh, 8, 4321, 0, 8, 1)
    assert np.array_equal(_bits(f), _bits(den)) and np.array_equal(_bits(v), _bits(var)) and np.array_equal(a, alb) and np.array_equal(n, nrm) and np.array_equal(z, dep)
    # spp = 1: the status of the C ABI
    film = np.zeros((Hh, W, 3), f32)
    assert jp.host_lib().jp_host_render_variance(be.h, W, Hh, 1, 5, 4321, 0, 1, 0, 0, 0, film.ctypes.data_as(C.c_void_p), None, None, None, None) == -1
