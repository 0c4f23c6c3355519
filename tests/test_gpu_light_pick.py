"""JP_LIGHTS_POWER_ONE on the MI355X (INTEGRATION.md "Light selection"): the device's table and pick are the definition, the degenerate case is
bit-exact, the estimator is unbiased and its weights do their job, more than 255 lights render, and the plumbing (shards, tone map, mode
switches, integrators, fused fallback, host API, command line) holds.  The statistics of tests 3 and 4 are recorded in DESIGN.md "Light selection"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
from test_light_table_host import check_table

pytestmark = pytest.mark.gpu
f32 = np.float32
W = Hh = 48
R_SPP = 4096


def _arr(p, n, dt=np.float32):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy() if n else np.zeros(0, dt)


@pytest.fixture()
def ctx():
    """a context of its own per test: the mode is context state, and the session's shared context must stay in JP_LIGHTS_ALL"""
    c = jp.Context(0)
    yield c
    c.close()


def _box(lamp, w=W, h=Hh, **kw):
    return scenes.build_lamp_box(scenes.HostBackend("lamp_box"), w, h, lamp, **kw)


def _film(ctx, be, mode, spp, seed=1234, depth=5, w=W, h=Hh, textured=False, **kw):
    ctx.set_light_sampling(mode)
    ctx.upload(be.flatten(), be.flatten_textures() if textured else None)
    return ctx.render(jp.render_params(w, h, spp, depth, seed, **kw))


def _weights(s):
    """the weights of the definition, in double from the fp32 scene values; areas in float32 with the upload's expressions"""
    n = s.n_lights
    ty = _arr(s.light_type, n, np.int32); rad = _arr(s.light_radiance, 3 * n).reshape(n, 3).astype(np.float64); lp = _arr(s.light_prim, n, np.int32)
    st, si = _arr(s.prim_shape_type, s.n_primitives, np.int32), _arr(s.prim_shape_index, s.n_primitives, np.int32)
    T = [_arr(getattr(s, "tri_p%d" % k), 3 * s.n_triangles).reshape(-1, 3) for k in range(3)]
    Q = [_arr(getattr(s, "rect_p%d" % k), 3 * s.n_rectangles).reshape(-1, 3) for k in range(3)]
    def cross_len(a, b):
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1).astype(f32)
        return np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]).astype(f32) + c[:, 2] * c[:, 2]).astype(f32)).astype(f32)
    w = np.zeros(n)
    for i in range(n):
        ssum = (rad[i, 0] + rad[i, 1]) + rad[i, 2]
        assert ty[i] == 1, "this test's scenes hold area lights only"
        p = lp[i]; k = si[p]
        if st[p] == 0:
            area = f32(0.5) * cross_len((T[1][k:k + 1] - T[0][k:k + 1]).astype(f32), (T[2][k:k + 1] - T[0][k:k + 1]).astype(f32))[0]
        else:
            assert st[p] == 1
            area = cross_len((Q[0][k:k + 1] - Q[1][k:k + 1]).astype(f32), (Q[2][k:k + 1] - Q[1][k:k + 1]).astype(f32))[0]
        w[i] = (ssum * float(area)) * np.pi
    return w


# ---- 1. the pick is the definition ----------------------------------------------------------------------------------------
def test_table_and_pick_are_the_definition(ctx):
    be = _box(scenes.lamp_66)
    s = be.flatten().contents
    assert s.n_lights == 66
    ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    w = _weights(s)
    assert len(np.unique(np.round(w[2:], 3))) > 16, "the mesh's triangles have unequal areas"
    q, alias, pmf = ctx.light_table()
    check_table(w, q, alias, pmf)
    info = ctx.light_info()
    assert (info.mode, info.n_lights, info.n_selectable) == (jp.JP_LIGHTS_POWER_ONE, 66, 66) and info.total_weight == float(np.cumsum(w)[-1])
    hq, ha, hp = jp.build_light_table(w)                               # the device holds what the host builder makes
    assert np.array_equal(q, hq) and np.array_equal(alias, ha) and np.array_equal(pmf, hp)
    rng = np.random.default_rng(5)
    last = f32(1.0 - 2.0 ** -24)
    u0 = np.concatenate([rng.random(4096, dtype=f32), [0, 0, last, last]]).astype(f32)
    u1 = np.concatenate([rng.random(4096, dtype=f32), [0, last, 0, last]]).astype(f32)
    idx, pm = ctx.light_pick(u0, u1)
    i = np.minimum((u0 * f32(66)).astype(np.int32), 65)
    j = np.where(u1 < q[i], i, alias[i])
    assert np.array_equal(idx, j) and np.array_equal(pm, pmf[j])
    assert len(np.unique(idx)) > 40


# ---- 2. bit-exact degenerate case --------------------------------------------------------------------------------------------
def _lit_and_black(be, m):
    scenes.lamp_rect()(be, m)
    be.pointlight((278, 273, -200), (0.0, 0.0, 0.0))


@pytest.mark.parametrize("textured", [False, True])
def test_one_lit_light_is_bit_exact(ctx, textured):
    """every draw of the debug sampler is 0.5, so the two extra draws move nothing; the black light has pmf 0, the lit one pmf 1"""
    be = _box(_lit_and_black, 32, 32, floor=(lambda b: b.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8))) if textured else None, full_materials=True)
    kw = dict(depth=5, w=32, h=32, textured=textured, sampler_mode=jp.JP_SAMPLER_DEBUG)
    a = _film(ctx, be, None, 2, **kw)
    assert ctx.light_info().picked_last_render == 0 and ctx.texture_info().textured_last_render == int(textured)
    b = _film(ctx, be, "power", 2, **kw)
    assert ctx.light_info().picked_last_render == 1 and ctx.texture_info().textured_last_render == int(textured)
    assert np.array_equal(ctx.light_table()[2], np.array([1, 0], f32))
    assert a.mean() > 0.02 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 3. / 4. unbiased, with the weights doing their job ------------------------------------------------------------------------
def _l2(film, R):
    """mean per-pixel L2 over the pixels where no channel of either film reaches 0.99 (Clamp01 biases those), and the share left out"""
    keep = (R < 0.99).all(-1) & (film < 0.99).all(-1)
    return float(np.sqrt(((film - R)[keep].astype(np.float64) ** 2).sum(-1)).mean()), 1.0 - keep.mean()


def _statistics(ctx, be, R, tag):
    assert 1.0 - (R < 0.99).all(-1).mean() <= 0.15
    e = {}
    for spp in (64, 1024):
        film = _film(ctx, be, "power", spp, seed=99)
        e[spp], out = _l2(film, R)
        assert out <= 0.15, (spp, out)
    films = [_film(ctx, be, "power", 128, seed=1000 + 17 * k) for k in range(8)]
    keep = (R < 0.99).all(-1)
    for f in films:
        keep &= (f < 0.99).all(-1)
    assert 1.0 - keep.mean() <= 0.15
    means = np.array([f[keep].astype(np.float64).mean() for f in films]); rmean = R[keep].astype(np.float64).mean()
    se = means.std(ddof=1) / np.sqrt(8.0)
    z = (means.mean() - rmean) / se
    print("%s: e(64) = %.5f, e(1024) = %.5f, ratio %.3f; image mean %.6f vs R %.6f, z = %+.2f (left out %.3f)" % (tag, e[64], e[1024], e[1024] / e[64], means.mean(), rmean, z, 1.0 - keep.mean()))
    assert e[1024] <= 0.35 * e[64], e                                   # an unbiased estimator: ~0.28 with R's own noise; a bias floor fails
    assert abs(z) <= 5.0, z


def test_66_lights_unbiased(ctx):
    be = _box(scenes.lamp_66)
    R = _film(ctx, be, None, R_SPP, seed=7)
    assert ctx.light_info().picked_last_render == 0
    _statistics(ctx, be, R, "66 lights")


def test_512_triangle_lamp(ctx):
    """more than 255 lights: refused as ever in ALL mode, rendered in POWER_ONE -- against the same lamp as ONE rectangle light"""
    R = _film(ctx, _box(scenes.lamp_rect()), None, R_SPP, seed=7)
    be = _box(scenes.lamp_mesh(16, 16))
    assert be.num_lights() == 512
    ctx.set_light_sampling(None)
    st = ctx.lib.jp_upload_scene(ctx.h, be.flatten())
    assert st == -5 and b"255 lights" in ctx.lib.jp_last_error()       # JP_ERR_UNSUPPORTED, today's message
    ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    info = ctx.light_info()
    assert info.n_lights == 512 and info.n_selectable == 512
    pmf = ctx.light_table()[2]
    assert np.allclose(pmf, 1.0 / 512, rtol=1e-5)
    _statistics(ctx, be, R, "512-triangle lamp")


# ---- 5. plumbing --------------------------------------------------------------------------------------------------------------
def test_shards_tone_map_and_mode_switches(ctx, H):
    be = _box(scenes.lamp_66)
    whole = _film(ctx, be, "power", 8)
    p = lambda **kw: jp.render_params(W, Hh, 8, 5, 1234, **kw)
    parts = [ctx.render(p(band_rows=5, shard_index=k, shard_count=3)) for k in range(3)]
    assert np.array_equal((parts[0] + parts[1] + parts[2]).view(np.uint32), whole.view(np.uint32))
    assert all((q_ == 0).all(-1).mean() > 0.5 for q_ in parts)
    rgb8, film = ctx.render_rgb8(p(), with_film=True)
    assert np.array_equal(film.view(np.uint32), whole.view(np.uint32))
    enc = np.zeros(film.size, np.uint8)
    jp.host_lib().jp_host_gamma_encode(film.ctypes.data_as(C.c_void_p), film.size, enc.ctypes.data_as(C.c_void_p))
    assert np.array_equal(rgb8.reshape(-1), enc)
    # the debug integrator ignores the mode, Whitted refuses it
    dbg = ctx.render(p(integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))
    assert ctx.light_info().picked_last_render == 0
    assert ctx.lib.jp_render(ctx.h, C.byref(p(integrator=jp.JP_INTEGRATOR_WHITTED)), dbg.ctypes.data_as(C.c_void_p)) == -5
    # the fused schedule falls back to the per-bounce launches, and the film is the same
    ctx.set_options(fused=1)
    fused = ctx.render(p())
    assert ctx.build_info().fused_last_render == 0 and ctx.light_info().picked_last_render == 1
    assert np.array_equal(fused.view(np.uint32), whole.view(np.uint32))
    ctx.set_options()
    # back to JP_LIGHTS_ALL: the Cornell box renders what a context that never heard of the mode renders
    hb = H.SCENES["cornell"](scenes.HostBackend("cornell"), W, Hh)
    ctx.set_light_sampling(None); ctx.upload(hb.flatten())
    back = ctx.render(p())
    assert ctx.light_info().picked_last_render == 0 and ctx.light_info().mode == jp.JP_LIGHTS_ALL
    fresh = jp.Context(0)
    fresh.upload(hb.flatten())
    today = fresh.render(p())
    fresh.close()
    assert np.array_equal(back.view(np.uint32), today.view(np.uint32))
    gold = np.load(os.path.join(H.GOLDEN, "film_cornell_counter.npy"))
    assert float(np.sqrt(((back - gold) ** 2).sum(-1)).mean()) < 1e-4
    assert ctx.lib.jp_get_light_table(ctx.h, None, None, None) == -5   # no table in ALL mode


def test_host_api_and_command_line(ctx, H, tmp_path):
    # FScene::SetLightSampling through the host library's integrator == the C ABI
    be = _box(scenes.lamp_mesh(16, 16))
    be.set_light_sampling("power")
    film = np.zeros((Hh, W, 3), f32); cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    direct = _film(ctx, be, "power", 4)
    assert film.mean() > 0.02 and np.array_equal(film.view(np.uint32), direct.view(np.uint32))
    be.set_light_sampling(None)                                        # ... and back: the 512 lights are refused again
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == -5
    # jetpbrt --light-sampling power
    root = scenes.export_reference_layout(str(tmp_path / "scene"), 24, 16)
    out = str(tmp_path / "cornell")
    r = subprocess.run([jp.CLI_PATH, "0", "8", "64", "48", "--assets", root, "--out", out, "--light-sampling", "power"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(out + ".bmp", "rb").read()
    img = np.frombuffer(raw[54:], np.uint8).reshape(48, 64, 3)[::-1, :, ::-1]
    hb = H.SCENES["cornell"](scenes.HostBackend("cornell"), 64, 48)
    p = jp.render_params(64, 48, 8, 5, 1234)
    ctx.set_light_sampling("power"); ctx.upload(hb.flatten())
    assert np.array_equal(img, ctx.render_rgb8(p))
    ctx.set_light_sampling(None); ctx.upload(hb.flatten())
    assert not np.array_equal(img, ctx.render_rgb8(p))
    r = subprocess.run([jp.CLI_PATH, "0", "1", "16", "16", "--light-sampling", "brightest"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 5
