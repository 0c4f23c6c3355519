"""Adaptive sampling on the MI355X (INTEGRATION.md "Adaptive sampling"): the device's list resolve, selection, compaction order and finish against the host
functions bit for bit (jp_adaptive_probe, no scene); ray generation through the list (every pixel of an adaptive render equals the uniform render of its own
sample count, bit for bit); the uniform render against the oracle-pinned jp_render within the rounding of one division; band shards, side effects, lens,
mip-mapped textures, the fused option, the refusals; and that at equal total samples the adaptive film is closer to a 4096-spp film than the uniform one."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import adaptive_ref as A

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = A.W, A.H                                                              # 40 x 24
MIN, STEP, MAX = 8, 8, 32
THR = 0.2                                                                    # relative standard error of the mean luminance at which a Cornell pixel stops
IMG = np.random.default_rng(3).integers(0, 256, (23, 37, 3), dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture()
def ctx():
    """a context of its own per test: the film state, the lens and the options are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _cornell(c, w=W, h=H):
    be = scenes.build_cornell(scenes.HostBackend("adaptive"), w, h, lambert_only=False)
    c.upload(be.flatten())
    return be


# ---- 1. probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 1])
def test_probe_equals_the_host_loop(ctx, dilate):
    """the cases of test_adaptive_host.py: survivor sets of 0, 1, 255, 256, 257, 959, 960 pixels (the compaction's wave, workgroup and tail boundaries), a short last
    pass, a film state with a sample clamp, hostile samples"""
    cases = [(A.synthetic_samples(A.survivor_pixels(k), 14), None, 4, 4, 0.05) for k in A.SURVIVORS]
    cases += [(A.synthetic_samples([p], 14), None, 4, 4, 0.05) for p in (0, W - 1, (H - 1) * W, 7 * W)]
    hostile = A.synthetic_samples(A.survivor_pixels(257), 14, hostile=True)
    hostile[::2, 100] = f32(3e30); hostile[1::2, 100] = 0
    cases += [(hostile, jp.film(hdr, clamp), 4, 4, 0.05) for hdr in (0, 1) for clamp in (0.0, 1.5)]
    rng = np.random.default_rng(11)
    sigma = (f32(10.0) ** rng.uniform(-2.5, 0, (1, H * W, 1))).astype(f32)
    cases += [(np.abs(f32(0.5) + sigma * rng.standard_normal((37, H * W, 3)).astype(f32)).astype(f32), jp.film(1, 0.0), 5, 6, 0.03)]
    for i, (s, film, mn, step, thr) in enumerate(cases):
        a = jp.adaptive(thr, mn, step, s.shape[0], 0.0, dilate)
        want = jp.adaptive_samples(film, a, s, H, W)
        got = ctx.adaptive_probe(a, s, H, W, film)
        bad = int((got[1] != want[1]).sum())
        if bad:
            print("probe case %d dilate %d: %d counts differ" % (i, dilate, bad))
        assert np.array_equal(got[1], want[1]), i
        assert np.array_equal(_bits(got[0]), _bits(want[0])), i
        assert np.array_equal(_bits(got[2]), _bits(want[2])), i
        info = ctx.adaptive_info()
        assert info.adaptive_last_render == 1 and info.samples_traced == int(want[1].sum()) and info.state_bytes_device >= 28 * H * W
    assert len(np.unique(want[1])) >= 4                                     # the last case stops pixels at several tests
    a = jp.adaptive(0.05, 4, 4, 0)
    assert ctx.lib.jp_adaptive_probe(ctx.h, None, C.byref(a), W, H, s.ctypes.data_as(C.c_void_p), None, want[1].ctypes.data_as(C.c_void_p), None) == -1


# ---- 2. ray generation through the list ---------------------------------------------------------------------------------------
def _check_against_uniform(c, rp, dilate, thr=THR):
    """the adaptive render; for every count n that occurs the uniform render min = max = n; bit equality on the pixels whose count is n.  The scene must adapt."""
    film, counts, var = c.render_adaptive(rp, jp.adaptive(thr, MIN, STEP, MAX, 0.0, dilate))
    assert c.counters().samples == int(counts.sum())
    values, share = np.unique(counts, return_counts=True)
    print("dilate %d thr %g: counts %s, pixels %s, passes %d" % (dilate, thr, values.tolist(), share.tolist(), c.adaptive_info().passes))
    assert set(values) <= {8, 16, 24, 32}
    assert (share >= 0.05 * counts.size).sum() >= 2, "fewer than two count values cover 5 % of the pixels each: the scene does not adapt at this threshold"
    assert (counts < MAX).any()
    uniform = {}
    for n in values:
        f, k, v = c.render_adaptive(rp, jp.adaptive(thr, int(n), STEP, int(n), 0.0, dilate))
        assert (k == n).all() and c.adaptive_info().passes == 1
        m = counts == n
        assert np.array_equal(_bits(film[m]), _bits(f[m])), n
        assert np.array_equal(_bits(var[m]), _bits(v[m])), n
        uniform[int(n)] = (f, v)
    return film, counts, var, uniform


@pytest.mark.parametrize("dilate", [0, 1])
def test_every_pixel_equals_the_uniform_render_of_its_count(ctx, dilate):
    _cornell(ctx)
    ctx.set_film(1)
    _check_against_uniform(ctx, jp.render_params(W, H, MAX, 5, 1234), dilate)


# ---- 3. against the existing path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 24, 32])
def test_uniform_render_against_jp_render(ctx, n):
    """min = max = n sums n non-negative fp32 samples and divides once; jp_render sums the same samples each scaled by fl(1 / n).  Relative to the exact mean the
    first is off by at most (n - 1) roundings of the sum + 1 of the division, the second by 1 of the ratio + n of the products + (n - 1) of the sum, each 2^-24:
    together below (2 n + 2) 2^-24 of the larger value (second-order terms are far below the slack of the two counts)."""
    _cornell(ctx)
    ctx.set_film(1)
    rp = jp.render_params(W, H, n, 5, 1234)
    a, counts, var = ctx.render_adaptive(rp, jp.adaptive(THR, n, STEP, 0, 0.0, 1))        # (max_spp 0: the render's spp)
    assert (counts == n).all() and ctx.counters().samples == n * W * H
    b = ctx.render(rp)
    err = np.abs(a.astype(np.float64) - b); bound = (2 * n + 2) * 2.0 ** -24 * np.maximum(a, b).astype(np.float64)
    print("n %d: max |a - b| / bound %.3f, %d of %d channels differ" % (n, (err[bound > 0] / bound[bound > 0]).max(), int((a != b).sum()), a.size))
    assert (err <= bound).all()
    _, v = ctx.render_variance(rp)
    assert np.array_equal(_bits(var), _bits(v))                              # the same recurrence on the same samples


# ---- 4. shards and state ----------------------------------------------------------------------------------------------------------
def test_shards_sum_to_the_whole(ctx):
    _cornell(ctx)
    ctx.set_film(1)
    a = jp.adaptive(THR, MIN, STEP, MAX, 0.0, 0)
    whole = ctx.render_adaptive(jp.render_params(W, H, MAX, 5, 1234, band_rows=4), a)
    parts = [ctx.render_adaptive(jp.render_params(W, H, MAX, 5, 1234, band_rows=4, shard_index=k, shard_count=2), a) for k in range(2)]
    rows = (np.arange(H) // 4) % 2 == 0
    assert (parts[0][1][~rows] == 0).all() and (parts[1][1][rows] == 0).all() and (parts[0][1][rows] >= MIN).all()
    assert np.array_equal(parts[0][1] + parts[1][1], whole[1])
    assert np.array_equal(_bits((parts[0][0] + parts[1][0]).astype(f32)), _bits(whole[0]))
    assert np.array_equal(_bits((parts[0][2] + parts[1][2]).astype(f32)), _bits(whole[2]))
    # dilate = 1 clips the neighbourhood to the shard: a shard's pixel never has fewer samples than without dilation
    d0 = parts[0][1]
    d1 = ctx.render_adaptive(jp.render_params(W, H, MAX, 5, 1234, band_rows=4, shard_index=0, shard_count=2), jp.adaptive(THR, MIN, STEP, MAX, 0.0, 1))[1]
    assert (d1 >= d0).all() and (d1[~rows] == 0).all() and (d1 > d0).any()


def test_a_render_after_an_adaptive_render_is_untouched(ctx):
    _cornell(ctx)
    rp = jp.render_params(W, H, 16, 5, 1234)
    fresh = jp.Context(0)
    try:
        _cornell(fresh)
        want = fresh.render(rp); want_v = fresh.render_variance(rp)[1]
    finally:
        fresh.close()
    b0 = jp.device_bytes_in_use()
    ctx.render_adaptive(rp, jp.adaptive(THR, MIN, 4, 0, 0.0, 1))
    info = ctx.adaptive_info()
    assert info.adaptive_last_render == 1 and info.passes >= 2 and info.state_bytes_device >= 28 * W * H and info.active_after[0] >= 0
    assert info.active_after[info.passes - 1] == -1 and ctx.build_info().lanes_last_render == 1
    assert np.array_equal(_bits(ctx.render(rp)), _bits(want))
    assert ctx.adaptive_info().adaptive_last_render == 0 and ctx.adaptive_info().passes == 0
    assert np.array_equal(_bits(ctx.render_variance(rp)[1]), _bits(want_v))
    ctx.render_adaptive(rp, jp.adaptive(THR, MIN, 4, 0, 0.0, 1))
    b1 = jp.device_bytes_in_use()
    ctx.render_adaptive(rp, jp.adaptive(THR, MIN, 4, 0, 0.0, 1))
    assert jp.device_bytes_in_use() == b1 and b1 >= b0                       # the per-pixel state lives for the length of the call


def test_lens_under_the_list(ctx):
    _cornell(ctx)
    ctx.set_film(1)
    ctx.set_lens(20.0, 900.0)
    _check_against_uniform(ctx, jp.render_params(W, H, MAX, 5, 1234), 1)
    assert ctx.lens_info().lens_last_render == 1


def test_mip_mapped_texture_under_the_list(ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("adaptive_tex"), W, H, back=lambda b: b.texture_image(IMG), floor=lambda b: b.texture_image(IMG))
    ctx.set_texture_sampling(be.flatten_texture_sampling())
    ctx.set_texture_mipmaps(jp.texture_mipmaps([1, 1], bounce_spread=0.125))
    ctx.upload(be.flatten(), be.flatten_textures())
    ctx.set_film(1)
    _check_against_uniform(ctx, jp.render_params(W, H, MAX, 5, 1234), 1)
    assert ctx.texture_mipmap_info().mip_last_render == 1


def test_fused_falls_back_and_whitted_refuses(ctx):
    _cornell(ctx)
    ctx.set_film(1)
    rp = jp.render_params(W, H, MAX, 5, 1234)
    a = jp.adaptive(THR, MIN, STEP, MAX, 0.0, 1)
    want = ctx.render_adaptive(rp, a)
    ctx.set_options(fused=1)
    try:
        ctx.render(rp)
        assert ctx.build_info().fused_last_render == 1                       # (the option is in force for jp_render)
        got = ctx.render_adaptive(rp, a)
        assert ctx.build_info().fused_last_render == 0
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g) if g.dtype == f32 else g, _bits(w) if w.dtype == f32 else w)
    finally:
        ctx.set_options()
    for integrator in (jp.JP_INTEGRATOR_WHITTED, jp.JP_INTEGRATOR_DEBUG_NORMAL):
        with pytest.raises(jp.JetPbrtError) as e:
            ctx.render_adaptive(jp.render_params(W, H, MAX, 5, 1234, integrator=integrator), a)
        assert "jp_render_adaptive" in str(e.value) and "path integrator" in str(e.value)
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.render_adaptive(rp, jp.adaptive(THR, 1, STEP, MAX))
    assert "min_spp" in str(e.value)
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.render_adaptive(jp.render_params(W, H, 4, 5, 1234), jp.adaptive(THR, MIN, STEP, 0))      # max_spp 0 -> spp = 4 < min_spp
    assert "max_spp" in str(e.value)
    again = ctx.render_adaptive(rp, a)                                       # the context stays usable
    assert np.array_equal(again[1], want[1]) and np.array_equal(_bits(again[0]), _bits(want[0]))


# ---- 5. it helps --------------------------------------------------------------------------------------------------------------------
def test_adaptive_beats_uniform_at_equal_samples(ctx):
    """Both films are compared with one 4096-spp film of jp_render (hdr).  The uniform render takes the adaptive render's rounded mean count per pixel, so the
    totals differ by less than half a sample per pixel.  The box's error is concentrated: the lamp, the directly lit walls and the floor converge within the
    first 8 samples, the indirect light under the boxes and the metal box's reflections do not; the adaptive render moves the samples of the first group to the
    second, whose squared error falls as 1 / n.  The 4096-spp film's own error is 1 / 4096 of a one-sample variance, two orders below either side."""
    w = h = 64
    _cornell(ctx, w, h)
    ctx.set_film(1)
    ref = ctx.render(jp.render_params(w, h, 4096, 5, 99)).astype(np.float64)
    film, counts, _ = ctx.render_adaptive(jp.render_params(w, h, 128, 5, 1234), jp.adaptive(THR / 2, 8, 8, 128, 0.0, 1))
    spp = int(round(float(counts.mean())))
    uni = ctx.render(jp.render_params(w, h, spp, 5, 1234))
    mse_a = float(((film - ref) ** 2).mean()); mse_u = float(((uni - ref) ** 2).mean())
    print("adaptive: mean count %.2f (uniform %d spp), counts %s; mse adaptive %.4e uniform %.4e ratio %.3f"
          % (counts.mean(), spp, dict(zip(*[x.tolist() for x in np.unique(counts, return_counts=True)])), mse_a, mse_u, mse_a / mse_u))
    assert 8 < counts.mean() < 128 and mse_a < mse_u


# ---- 6. the host API -------------------------------------------------------------------------------------------------------------------
def test_host_api_counts_and_the_variance_guided_filter(ctx):
    """FFilm::SetAdaptive / SampleCounts / Variance through FGpuPathIntegrator::Render equal the C ABI's planes; with RequestDenoise(n, { varianceGuided }) the film is
    jp_denoise_variance of that film, the guides of jp_render_guides and the adaptive render's own variance plane"""
    be = _cornell(ctx)
    ctx.set_film(1)
    rp = jp.render_params(W, H, MAX, 5, 1234)
    want = ctx.render_adaptive(rp, jp.adaptive(THR, MIN, STEP, MAX, 0.0, 1))
    L = jp.host_lib()
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    film = np.zeros((H, W, 3), f32); counts = np.zeros((H, W), np.int32); var = np.zeros((H, W), f32)
    assert L.jp_host_render_adaptive(be.h, W, H, MAX, 5, 1234, 0, THR, MIN, STEP, 1, 0, 0, 1, q(film), q(counts), q(var)) == 0
    assert np.array_equal(counts, want[1]) and np.array_equal(_bits(film), _bits(want[0])) and np.array_equal(_bits(var), _bits(want[2]))
    den = np.zeros((H, W, 3), f32)
    assert L.jp_host_render_adaptive(be.h, W, H, MAX, 5, 1234, 0, THR, MIN, STEP, 1, 4, 1, 1, q(den), q(counts), q(var)) == 0
    alb, nrm, dep = ctx.render_guides(rp, 4)
    out, _ = ctx.denoise_variance(want[0], alb, nrm, dep, want[2])
    assert np.array_equal(_bits(den), _bits(out)) and not np.array_equal(_bits(den), _bits(film)) and np.array_equal(counts, want[1])
    assert L.jp_host_render_adaptive(be.h, W, H, MAX, 5, 1234, 0, THR, 1, STEP, 1, 0, 0, 1, q(film), q(counts), q(var)) != 0      # min_spp 1: refused, nothing delivered
