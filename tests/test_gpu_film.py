"""The film on the MI355X (INTEGRATION.md "Film"): nothing set is a no-op, exact HDR values, the clamp identity over the integrators and additive features, batches
and schedules, the sample clamp, the luminance histogram against numpy, the display transform against the host function and numpy bit for bit, the one-call
renders against the separate calls, the HDR denoise, device memory, the host API.  Frames are 32 x 24 at <= 8 spp."""
import ctypes as C
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import denoise_ref as DR
import film_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
W, Hh = 32, 24
CURVES = [jp.JP_CURVE_CLAMP, jp.JP_CURVE_REINHARD, jp.JP_CURVE_ACES, jp.JP_CURVE_HABLE]


@pytest.fixture()
def ctx():
    """a context of its own per test: film state and tone map are context state"""
    c = jp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell():
    be = scenes.build_cornell(scenes.HostBackend("film_cornell"), W, Hh, lambert_only=False)
    return be, be.flatten()


@pytest.fixture(scope="module")
def hdr_film(cornell):
    """the HDR Cornell film at 8 spp (the lamp is in view: values above 1) and its clamped twin, rendered once"""
    c = jp.Context(0)
    c.upload(cornell[1])
    p = jp.render_params(W, Hh, 8, 5, 1234)
    ldr = c.render(p)
    c.set_film(1)
    hdr = c.render(p)
    assert c.film_info().hdr_last_render == 1
    c.close()
    hdr.setflags(write=False); ldr.setflags(write=False)
    return hdr, ldr


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _has_highlights(hdr):
    """the precondition of the clamp tests: something above 1 to cut off, something strictly inside (0, 1) to leave alone"""
    return bool((hdr > 1).any() and ((hdr > 0) & (hdr < 1)).any())


def _adversarial_film():
    v = R.adversarial_values()
    return v.reshape(1, -1, 3)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_set_equals_a_fresh_context(ctx, cornell):
    p = jp.render_params(W, Hh, 8, 5, 1234)
    fresh = jp.Context(0)
    fresh.upload(cornell[1])
    b0, f0 = fresh.render_rgb8(p, with_film=True)
    fresh.close()
    ctx.upload(cornell[1])
    ctx.set_film(1, 2.0); ctx.set_tonemap("aces", exposure="auto")
    b1, f1 = ctx.render_rgb8(p, with_film=True)
    assert ctx.film_info().hdr_last_render == 1 and ctx.tonemap_info().mapped_last_render == 1 and not _same(f1, f0)
    ctx.set_film(None); ctx.set_tonemap(None)
    b2, f2 = ctx.render_rgb8(p, with_film=True)
    fi, ti = ctx.film_info(), ctx.tonemap_info()
    assert _same(f2, f0) and np.array_equal(b2, b0)
    assert fi.hdr == 0 and fi.sample_clamp == 0 and fi.hdr_last_render == 0 and ti.mapped_last_render == 0 and ti.curve == 0 and ti.exposure_mode == 0
    # {hdr 0, sample_clamp 0} is no film state either
    ctx.set_film(0, 0.0)
    assert _same(ctx.render(p), f0) and ctx.film_info().hdr_last_render == 0
    # a refused state leaves the one in force
    ctx.set_film(1, 3.0)
    bad = jp.film(1, float("nan"))
    assert ctx.lib.jp_set_film(ctx.h, C.byref(bad)) == -1 and ctx.film_info().sample_clamp == 3.0
    badt = jp.tonemap(7)
    ctx.set_tonemap("hable")
    assert ctx.lib.jp_set_tonemap(ctx.h, C.byref(badt)) == -1 and ctx.tonemap_info().curve == jp.JP_CURVE_HABLE


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [4, 1])
def test_exact_hdr_value(ctx, spp):
    """a rectangle emitter of radiance (7, 3, 0.5) that fills the view, nothing else: every sample is that radiance, and the sum of spp terms l * (1 / spp) is exact"""
    be = scenes.HostBackend("film_emitter")
    be.camera((0.0, 0.0, 10.0), (0, 0, -1), (0, 1, 0), 60.0, W, Hh)
    be.rect(scenes.AXIS_XY, -100.0, 100.0, -100.0, 100.0, 0.0, False, be.mat_matte((0.0, 0.0, 0.0)), (7.0, 3.0, 0.5))
    be.preprocess()
    ctx.upload(be.flatten())
    p = jp.render_params(W, Hh, spp, 5, 99)
    ldr = ctx.render(p)
    ctx.set_film(1)
    hdr = ctx.render(p)
    assert _same(hdr, np.broadcast_to(np.array([7.0, 3.0, 0.5], f32), (Hh, W, 3)))
    assert _same(ldr, np.broadcast_to(np.array([1.0, 1.0, 0.5], f32), (Hh, W, 3)))


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def _clamp_identity(ctx, p):
    ctx.set_film(None)
    ldr = ctx.render(p)
    ctx.set_film(1)
    hdr = ctx.render(p)
    assert ctx.film_info().hdr_last_render == 1
    assert _has_highlights(hdr), "the scene must show its lamp (values above 1) and lit surfaces (values inside (0, 1))"
    assert _same(np.clip(hdr, f32(0), f32(1)), ldr)


def test_clamp_identity_path(hdr_film):
    hdr, ldr = hdr_film
    assert _has_highlights(hdr) and _same(np.clip(hdr, f32(0), f32(1)), ldr)


def test_clamp_identity_whitted(ctx, cornell):
    ctx.upload(cornell[1])
    _clamp_identity(ctx, jp.render_params(W, Hh, 4, 5, 1234, integrator=jp.JP_INTEGRATOR_WHITTED))


def test_clamp_identity_power_mis(ctx, cornell):
    ctx.set_light_sampling("power")
    ctx.upload(cornell[1])
    ctx.set_estimator("mis")
    _clamp_identity(ctx, jp.render_params(W, Hh, 8, 5, 1234))
    assert ctx.estimator_info().mis_last_render == 1


def test_clamp_identity_textured(ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("film_textured"), W, Hh, floor=lambda b: b.texture_checker((0.8, 0.8, 0.1), (0.1, 0.2, 0.8)))
    ctx.upload(be.flatten(), be.flatten_textures())
    _clamp_identity(ctx, jp.render_params(W, Hh, 8, 5, 1234))
    assert ctx.texture_info().textured_last_render == 1


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_batches_and_schedules(ctx, cornell, hdr_film):
    hdr = hdr_film[0]
    ctx.upload(cornell[1])
    ctx.set_film(1)
    p = jp.render_params(W, Hh, 8, 5, 1234)
    ctx.set_options(lanes=1, max_slots=8 * W * Hh)                 # the frame once: one batch
    assert _same(ctx.render(p), hdr)
    ctx.set_options(); ctx.set_options(lanes=1, max_slots=2 * W * Hh)   # four batches: the running sum lives in pix_acc
    assert _same(ctx.render(p), hdr)
    ctx.set_options(); ctx.set_options(lanes=2)
    assert _same(ctx.render(p), hdr) and ctx.build_info().lanes_last_render == 2
    ctx.set_options(); ctx.set_options(fused=1)
    assert _same(ctx.render(p), hdr) and ctx.build_info().fused_last_render == 1 and ctx.film_info().hdr_last_render == 1
    ctx.set_options(); ctx.set_options(fused=1, max_slots=2 * W * Hh)
    assert _same(ctx.render(p), hdr) and ctx.build_info().fused_last_render == 1
    ctx.set_options()
    # band shards sum to the full HDR film
    shards = [ctx.render(jp.render_params(W, Hh, 8, 5, 1234, band_rows=4, shard_index=k, shard_count=3)) for k in range(3)]
    assert all(s.any() for s in shards) and _same(shards[0] + shards[1] + shards[2], hdr)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_sample_clamp(ctx, cornell):
    c = 2.0
    ctx.upload(cornell[1])
    p1 = jp.render_params(W, Hh, 1, 5, 1234)
    ctx.set_film(1)
    raw = ctx.render(p1)                                           # at 1 spp the film is the sample: L = 0 + l * 1.0f
    assert (raw.max(axis=-1) > c).any(), "some sample must exceed the clamp"
    ctx.set_film(1, c)
    got = ctx.render(p1)
    assert _same(got.reshape(-1, 3), jp.film_samples(jp.film(1, c), raw.reshape(-1, 3)))
    assert _same(got.reshape(-1, 3), R.sample_clamp(c, raw.reshape(-1, 3))) and not _same(got, raw)
    # ... and with hdr 0 the clamped samples meet Clamp01 afterwards
    ctx.set_film(0, c)
    assert _same(ctx.render(p1), np.clip(got, f32(0), f32(1))) and ctx.film_info().hdr_last_render == 1
    # 8 spp: eight roundings of a sum of terms <= c / 8
    p8 = jp.render_params(W, Hh, 8, 5, 1234)
    ctx.set_film(1); free = ctx.render(p8)
    ctx.set_film(1, c); tame = ctx.render(p8)
    assert tame.max() <= c * (1 + 8 * 2.0 ** -24) and free.max() > c and not _same(tame, free)
    # the schedules agree on it
    ctx.set_options(fused=1)
    assert _same(ctx.render(p8), tame) and ctx.build_info().fused_last_render == 1
    ctx.set_options(); ctx.set_options(lanes=2, max_slots=2 * W * Hh)
    assert _same(ctx.render(p8), tame)
    ctx.set_options()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------------
def _synthetic(npix, seed):
    rng = np.random.default_rng(seed)
    return (2.0 ** rng.uniform(-34.0, 33.0, (1, npix, 3))).astype(f32)


class _DeviceBuffer:
    """device memory through the HIP runtime the library is linked against"""
    def __init__(self, lib, nbytes):
        self.lib, self.p = lib, C.c_void_p()
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert lib.hipMalloc(C.byref(self.p), nbytes) == 0
    def put(self, a):
        assert self.lib.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    def get(self, a):
        assert self.lib.hipMemcpy(a.ctypes.data_as(C.c_void_p), self.p, a.nbytes, 2) == 0
        return a
    def free(self):
        self.lib.hipFree(self.p)


@pytest.mark.parametrize("npix", [1, 63, 64, 65, 257, 256 * 8 * 3 + 1])
def test_histogram_synthetic_sizes(ctx, npix):
    """lane, wave, workgroup and grid-stride tails"""
    film = _synthetic(npix, npix)
    h = ctx.film_histogram(film)
    assert h.dtype == np.uint32 and np.array_equal(h, R.histogram(film)) and int(h.sum()) == npix


def test_histogram_rendered_uniform_adversarial_and_device_pointers(ctx, hdr_film):
    hdr = hdr_film[0]
    h = ctx.film_histogram(hdr)
    assert np.array_equal(h, R.histogram(hdr)) and int(h.sum()) == W * Hh and np.count_nonzero(h[:R.BINS]) > 8
    # one repeated value: every lane of every wave adds to one LDS counter
    uni = np.broadcast_to(np.array([0.7, 0.5, 0.3], f32), (64, 64, 3))
    hu = ctx.film_histogram(uni)
    assert np.array_equal(hu, R.histogram(uni)) and hu.max() == 64 * 64
    black = np.zeros((64, 64, 3), f32)
    assert ctx.film_histogram(black)[R.BINS] == 64 * 64
    # zeros, negatives, non-finite values: excluded; the out-of-range ends: bins 0 and 255
    adv = _adversarial_film()
    ha = ctx.film_histogram(adv)
    assert np.array_equal(ha, R.histogram(adv)) and ha[R.BINS] > 0 and ha[0] > 0 and ha[255] > 0
    # the device-pointer entry point
    for film in (np.ascontiguousarray(hdr), np.ascontiguousarray(adv)):
        d_film = _DeviceBuffer(ctx.lib, film.nbytes); d_hist = _DeviceBuffer(ctx.lib, 4 * (R.BINS + 1))
        d_film.put(film); d_hist.put(np.full(R.BINS + 1, 0xdeadbeef, np.uint32))       # the call zeroes the counters itself
        ctx.film_histogram_device(film.shape[1], film.shape[0], d_film.p.value, d_hist.p.value, sync=True)
        got = d_hist.get(np.zeros(R.BINS + 1, np.uint32))
        d_film.free(); d_hist.free()
        assert np.array_equal(got, ctx.film_histogram(film))
    assert ctx.tonemap_info().histogram_ms > 0


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_display_transform_is_the_host_function(ctx, curve):
    adv = _adversarial_film()
    thr = np.zeros(255, f32)
    assert ctx.lib.jp_gamma_thresholds(thr.ctypes.data_as(C.c_void_p)) == 0
    for ev in (-2.0, 0.0, 3.0):
        t = jp.tonemap(curve, "manual", ev)
        b, y, scale = ctx.tonemap(adv, t)
        assert scale == 2.0 ** ev
        hb, hy = jp.tonemap_host(t, scale, adv)
        want = R.curve_values(t, scale, adv)
        assert _same(y, hy) and np.array_equal(b, hb), (curve, ev)
        assert _same(y, want) and np.array_equal(b, R.gamma_bytes(thr, want)), (curve, ev)
    # bytes alone, floats alone; the tone map in force when none is given
    t = jp.tonemap(curve, "manual", 1.0, white=2.0)
    ctx.set_tonemap(t)
    b, none, _ = ctx.tonemap(adv, want_floats=False)
    none2, y, _ = ctx.tonemap(adv, want_bytes=False)
    hb, hy = jp.tonemap_host(t, 2.0, adv)
    assert none is None and none2 is None and np.array_equal(b, hb) and _same(y, hy)
    ctx.set_tonemap(None)
    assert ctx.lib.jp_tonemap(ctx.h, None, 4, 4, adv.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), None, None) == -1     # none given, none in force


def test_clamp_manual_ev0_gives_render_rgb8_bytes(ctx, cornell):
    ctx.upload(cornell[1])
    p = jp.render_params(W, Hh, 4, 5, 7)
    b0, f0 = ctx.render_rgb8(p, with_film=True)                    # k_tonemap8
    ctx.set_tonemap("clamp")
    b1, f1 = ctx.render_rgb8(p, with_film=True)                    # k_display<CLAMP>
    assert ctx.tonemap_info().mapped_last_render == 1 and _same(f1, f0) and np.array_equal(b1, b0)
    ctx.set_film(1)
    b2, f2 = ctx.render_rgb8(p, with_film=True)                    # ... on the HDR film: the clamp is the curve's
    assert (f2 > 1).any() and np.array_equal(b2, b0)


def test_auto_exposure_scale_is_the_host_function(ctx, hdr_film):
    hdr = hdr_film[0]
    hist = ctx.film_histogram(hdr)
    for t in (jp.tonemap("aces", "auto"), jp.tonemap("reinhard", "auto", 1.0, key=0.36, pct_low=0.2, pct_high=0.8)):
        b, y, scale = ctx.tonemap(hdr, t)
        assert scale == jp.exposure_from_histogram(t, hist) and scale != 1.0
        hb, hy = jp.tonemap_host(t, scale, hdr)
        assert _same(y, hy) and np.array_equal(b, hb)
        assert ctx.tonemap_info().scale_last == scale
    # the device-pointer entry point gives the same floats and bytes
    t = jp.tonemap("hable", "auto")
    film = np.ascontiguousarray(hdr)
    d_film = _DeviceBuffer(ctx.lib, film.nbytes); d_rgb = _DeviceBuffer(ctx.lib, film.nbytes); d_b = _DeviceBuffer(ctx.lib, film.size)
    d_film.put(film)
    scale = ctx.tonemap_device(W, Hh, d_film.p.value, d_b.p.value, d_rgb.p.value, t, sync=True)
    y = d_rgb.get(np.zeros_like(film)); b = d_b.get(np.zeros(film.shape, np.uint8))
    d_film.free(); d_rgb.free(); d_b.free()
    hb, hy, hs = ctx.tonemap(film, t)
    assert scale == hs and _same(y, hy) and np.array_equal(b, hb)


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_one_call_equals_the_separate_calls(ctx, cornell, hdr_film):
    ctx.upload(cornell[1])
    ctx.set_film(1); ctx.set_tonemap("aces", exposure="auto")
    p = jp.render_params(W, Hh, 8, 5, 1234)
    b, film = ctx.render_rgb8(p, with_film=True)
    ti = ctx.tonemap_info()
    assert _same(film, hdr_film[0]) and ti.mapped_last_render == 1 and ti.curve == jp.JP_CURVE_ACES and ti.exposure_mode == jp.JP_EXPOSURE_AUTO
    wb, _, scale = ctx.tonemap(film)
    assert np.array_equal(b, wb) and ti.scale_last == scale
    # render -> guides -> denoise -> tone map, chained by hand
    f2, b2, alb, nrm, dep = ctx.render_denoised(p, guide_spp=4, iterations=3)
    assert ctx.tonemap_info().mapped_last_render == 1
    galb, gnrm, gdep = ctx.render_guides(p, 4)
    den = ctx.denoise(film, galb, gnrm, gdep, iterations=3)
    wb2, _, _ = ctx.tonemap(den)
    assert _same(alb, galb) and _same(nrm, gnrm) and _same(dep, gdep) and _same(f2, den) and np.array_equal(b2, wb2)
    assert (den > 1).any()
    # guides only: the film as rendered, its bytes through the tone map
    f3, b3, _, _, _ = ctx.render_denoised(p, guide_spp=4, denoise=False)
    assert _same(f3, film) and np.array_equal(b3, b)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [True, False])
def test_hdr_denoise(ctx, demod):
    Hd, Wd = 40, 67                                                # no multiple of the 32 x 8 tile
    film, albedo, normal, depth = DR.filter_inputs(Hd, Wd, 5)
    film = (film * f32(8.0)).astype(f32)                           # radiance up to 8
    kw = dict(iterations=3, sigma_color=2.0, sigma_normal=0.3, sigma_depth=0.1, demodulate=1 if demod else -1)
    ref = dict(iterations=3, sigma_color=2.0, sigma_normal=0.3, sigma_depth=0.1, demodulate=demod)
    ctx.set_film(1)
    out = ctx.denoise(film, albedo, normal, depth, **kw)
    assert _same(out, R.atrous_hdr_ref(film, albedo, normal, depth, **ref)) and (out > 1).any() and out.min() >= 0
    ctx.set_film(0, 5.0)                                           # a sample clamp alone is no HDR: the filter clamps as ever
    clamped = ctx.denoise(film, albedo, normal, depth, **kw)
    assert _same(clamped, DR.atrous_ref(film, albedo, normal, depth, **ref)) and clamped.max() <= 1
    ctx.set_film(None)
    assert _same(ctx.denoise(film, albedo, normal, depth, **kw), clamped)
    assert _same(np.clip(out, f32(0), f32(1)), clamped)


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_memory_returns_to_its_starting_value(cornell):
    start = jp.device_bytes_in_use()
    c = jp.Context(0)
    c.upload(cornell[1])
    c.set_film(1, 4.0); c.set_tonemap("hable", exposure="auto")
    p = jp.render_params(W, Hh, 4, 5, 3)
    b, film = c.render_rgb8(p, with_film=True)
    c.film_histogram(film); c.tonemap(film); c.render_denoised(p, guide_spp=2, iterations=2)
    assert jp.device_bytes_in_use() > start
    c.close()
    assert jp.device_bytes_in_use() == start


# ---- 11 ---------------------------------------------------------------------------------------------------------------------------------------------
def _read_hdr(path):
    raw = open(path, "rb").read()
    head, _, rest = raw.partition(b"\n\n")
    assert head.startswith(b"#?RADIANCE")
    res, _, px = rest.partition(b"\n")
    _, h, _, w = res.split()
    a = np.frombuffer(px, np.uint8).reshape(int(h), int(w), 4).astype(np.float64)
    return a[..., :3] * np.where(a[..., 3:] > 0, 2.0 ** (a[..., 3:] - 136.0), 0.0)


def _read_ppm(path):
    tok = open(path).read().split()
    assert tok[0] == "P3" and tok[3] == "255"
    return np.array(tok[4:], np.int64).reshape(int(tok[2]), int(tok[1]), 3).astype(np.uint8)


def test_host_api(ctx, cornell, hdr_film, tmp_path):
    be, sp = cornell
    ctx.upload(sp)
    ctx.set_film(1); ctx.set_tonemap("aces", exposure="auto")
    want_b, want_f = ctx.render_rgb8(jp.render_params(W, Hh, 8, 5, 1234), with_film=True)
    want_scale = ctx.tonemap_info().scale_last
    L = jp.host_lib()
    film = np.zeros((Hh, W, 3), f32); rgb8 = np.zeros((Hh, W, 3), np.uint8); scale = C.c_float(0)
    q = lambda a: a.ctypes.data_as(C.c_void_p)
    # FFilm::SetToneMap turns HDR on; the .hdr file holds the unclamped film
    name = str(tmp_path / "film")
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 0, 0.0, 1, jp.JP_CURVE_ACES, 1, 0.0, 0.0, 0, q(film), q(rgb8), C.byref(scale), name.encode(), 2) == 0
    assert _same(film, want_f) and _same(film, hdr_film[0]) and np.array_equal(rgb8, want_b) and scale.value == want_scale
    dec = _read_hdr(name + ".hdr")
    assert dec.shape == (Hh, W, 3) and dec.max() > 1 and abs(dec.max() - film.max()) <= film.max() / 128      # RGBE: 8 bits of mantissa
    # the .ppm goes through the tone map: next to the fp32 film, and instead of it (RequestDeviceLDR)
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 0, 0.0, 1, jp.JP_CURVE_ACES, 1, 0.0, 0.0, 0, None, None, None, name.encode(), 0) == 0
    assert np.array_equal(_read_ppm(name + ".ppm"), want_b)
    os.remove(name + ".ppm")
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 0, 0.0, 1, jp.JP_CURVE_ACES, 1, 0.0, 0.0, 1, None, q(rgb8), None, name.encode(), 0) == 0
    assert np.array_equal(_read_ppm(name + ".ppm"), want_b) and np.array_equal(rgb8, want_b)
    # SetHDR alone: the unclamped film, no bytes; a film that asks for nothing renders as ever (the integrator takes the state back)
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 1, 0.0, 0, 0, 0, 0.0, 0.0, 0, q(film), None, None, None, 0) == 0
    assert _same(film, hdr_film[0])
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 0, 0.0, 0, 0, 0, 0.0, 0.0, 0, q(film), None, None, None, 0) == 0
    assert _same(film, hdr_film[1])
    # SetSampleClamp reaches the device
    assert L.jp_host_render_film(be.h, W, Hh, 8, 5, 1234, 0, 1, 2.0, 0, 0, 0, 0.0, 0.0, 0, q(film), None, None, None, 0) == 0
    assert film.max() <= 2.0 * (1 + 8 * 2.0 ** -24) and film.max() > 1
