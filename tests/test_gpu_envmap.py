"""Environment maps on the MI355X (INTEGRATION.md "Environment maps"): the device's lookup and sample are the definition, the sky is the image bit
for bit, the estimator is unbiased against a closed form and its importance sampling does its job, a constant map is the constant light, and the
plumbing (shards, lanes, tone map, textures, refusals, fused fallback, clearing the map, memory, host API, command line) holds.  The restatement is
tests/envmap_ref.py; the figures these tests print are recorded in DESIGN.md "Environment maps"."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import envmap_ref as E

pytestmark = pytest.mark.gpu
f32 = np.float32
TINT = (0.5, 1.0, 0.75)
UPS = [("z", E.UP_Z), ("y", E.UP_Y)]


@pytest.fixture()
def ctx():
    """a context of its own per test: the map and the light sampling mode are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _upload(ctx, be, rgb, up="z", importance=0, mode="power", textured=False):
    ctx.set_environment_map(rgb, up, importance)
    ctx.set_light_sampling(mode)
    ctx.upload(be.flatten(), be.flatten_textures() if textured else None)


def _probe_scene(tint=TINT):
    """one small matte rectangle and the environment light: what the lookup / sample probes need"""
    be = scenes.HostBackend("envmap_probe")
    be.camera((0, 0, 0), (1, 0, 0), (0, 0, 1), 60.0, 16, 16)
    be.envlight(tint)
    be.rect(scenes.AXIS_YZ, -1, 1, -1, 1, -5.0, False, be.mat_matte((0.5, 0.5, 0.5)))
    be.preprocess()
    return be


# ---- 1. lookup and sample are the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,upc", UPS)
def test_lookup_and_sample_are_the_definition(ctx, up, upc):
    rgb = E.bright_map(); Hh, W = rgb.shape[:2]
    _upload(ctx, _probe_scene(), rgb, up)
    t = jp.build_environment_table(rgb, TINT)
    info = ctx.env_info()
    assert (info.width, info.height, info.up_axis, info.importance, info.n_selectable) == (W, Hh, upc, 0, W * (Hh - 1))
    assert info.total_weight == t["total"] and info.mean_sum == t["mean_sum"] and info.table_bytes_device >= W * Hh * 24 + Hh * 8
    rng = np.random.default_rng(7)
    last = f32(1.0 - 2.0 ** -24)
    corners = np.array([[a0, a1, a2, b0, b1] for a0 in (0, last) for a1 in (0, last) for a2 in (0, last) for b0 in (0, last) for b1 in (0, last)], f32)
    u = np.concatenate([rng.random((4096, 5), dtype=f32), corners]).astype(f32)
    idx, wi, Li, pdf = ctx.env_sample(u)
    j, wref = E.sample(u, t["q"], t["alias"], W, Hh, upc)
    assert np.array_equal(idx, j)                                      # (int) of fp32 products and table loads only
    assert np.array_equal(Li.view(np.uint32), t["texel"][j, :3].view(np.uint32)) and np.array_equal(pdf.view(np.uint32), t["texel"][j, 3].view(np.uint32))
    dmax = float(np.abs(wi.astype(np.float64) - wref).max()); nmax = float(np.abs(np.linalg.norm(wi.astype(np.float64), axis=-1) - 1.0).max())
    print("up %s: largest |wi - restatement| = %.3e, largest | |wi| - 1 | = %.3e" % (up, dmax, nmax))
    assert dmax <= 4e-6 and nmax <= 1e-6
    assert len(np.unique(idx)) > 40 and (t["weight"][idx] > 0).all()
    # lookup: texel centres exactly; random directions exactly away from the borders
    ct, cb = E.row_cos(Hh)
    r, c = np.divmod(np.arange(W * Hh), W)
    th = np.pi * (r + 0.5) / Hh; ph = 2.0 * np.pi * (c + 0.5) / W
    centres = E.to_world(np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1), upc).astype(f32)
    li, lrgb = ctx.env_lookup(centres)
    assert np.array_equal(li, np.arange(W * Hh)) and np.array_equal(lrgb.view(np.uint32), t["texel"][:, :3].view(np.uint32))
    d = rng.normal(size=(4096, 3)); d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    li, _ = ctx.env_lookup(d)
    ref, border = E.lookup(d, W, Hh, upc)
    keep = border >= 1e-3
    print("up %s: %.2f %% of the random directions within 1e-3 of a border" % (up, 100.0 * (1.0 - keep.mean())))
    assert 1.0 - keep.mean() <= 0.02 and np.array_equal(li[keep], ref[keep])
    back, _ = ctx.env_lookup(wi)
    print("up %s: a lookup of the sampled wi returns the sampled texel for %.2f %%" % (up, 100.0 * (back == idx).mean()))
    assert (back == idx).mean() >= 0.98


# ---- 2. the sky is the image, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,upc", UPS)
def test_sky_is_the_image(ctx, up, upc):
    rng = np.random.default_rng(21)
    rgb = rng.uniform(0.05, 0.95, (2, 4, 3)).astype(f32)
    be = scenes.HostBackend("envmap_sky")
    front = scenes._normalize((1.0, 0.0, 0.0) if upc == E.UP_Z else (0.0, 0.0, 1.0))       # along the horizon, at the seam phi = 0
    be.camera((0, 0, 0), front, (0, 0, 1) if upc == E.UP_Z else (0, 1, 0), 60.0, 16, 16)
    be.envlight(TINT)
    m = be.mat_matte((0.5, 0.5, 0.5))
    if upc == E.UP_Z:
        be.rect(scenes.AXIS_YZ, -1, 1, -1, 1, -5.0, False, m)         # behind the camera
    else:
        be.rect(scenes.AXIS_XY, -1, 1, -1, 1, -5.0, False, m)
    be.preprocess()
    _upload(ctx, be, rgb, up)
    film = ctx.render(jp.render_params(16, 16, 1, 5, 1234, sampler_mode=jp.JP_SAMPLER_DEBUG))
    assert ctx.env_info().mapped_last_render == 1
    cam = be.flatten().contents.camera
    fr, ri, upv = (np.array(list(v), np.float64) for v in (cam.front, cam.right, cam.up))
    x, y = np.meshgrid(np.arange(16) + 0.5, np.arange(16) + 0.5)
    d = fr[None, None] + ri[None, None] * (x / 16.0 - 0.5)[..., None] + upv[None, None] * (0.5 - y / 16.0)[..., None]
    ref, border = E.lookup(d.reshape(-1, 3), 4, 2, upc)
    keep = (border >= 1e-3).reshape(16, 16)
    assert 1.0 - keep.mean() <= 0.05
    want = E.tinted(rgb, TINT).reshape(-1, 3)[ref].reshape(16, 16, 3)
    assert len(np.unique(ref)) == 4, "the film sees both rows and two columns"
    assert np.array_equal(film[keep].view(np.uint32), want[keep].view(np.uint32))


# ---- 3. / 4. unbiased against the closed form, with the importance doing its job -----------------------------------------------------------
KD = (0.8, 0.7, 0.6)
FLOOR_TARGET = 0.559               # the closed form's largest channel after scaling the map


def _floor():
    be = scenes.HostBackend("envmap_floor")
    be.camera((0, 5, 0), (0, -1, 0), (0, 0, -1), 40.0, 32, 32)
    be.envlight((1.0, 1.0, 1.0))
    be.rect(scenes.AXIS_XZ, -50, 50, -50, 50, 0.0, False, be.mat_matte(KD))
    be.preprocess()
    return be


def _floor_map():
    rgb = E.bright_map()
    return (rgb * f32(FLOOR_TARGET / E.floor_closed_form(rgb, (1, 1, 1), KD).max())).astype(f32)


def test_unbiased_against_closed_form(ctx):
    rgb = _floor_map()
    expected = E.floor_closed_form(rgb, (1, 1, 1), KD)
    print("closed form: %s" % np.array2string(expected, precision=5))
    assert abs(expected.max() - FLOOR_TARGET) < 1e-4
    _upload(ctx, _floor(), rgb, "y")
    films = [ctx.render(jp.render_params(32, 32, 128, 1, 1000 + 17 * k)) for k in range(8)]
    assert ctx.env_info().mapped_last_render == 1
    top = max(float(f.max()) for f in films)
    print("largest pixel value of the eight films: %.4f" % top)
    assert top < 0.99                                                   # no pixel clamped (Clamp01 would bias the mean); nothing is masked
    means = np.array([f.astype(np.float64).mean((0, 1)) for f in films])          # (8, 3)
    se = means.std(0, ddof=1) / np.sqrt(8.0)
    z = (means.mean(0) - expected) / se
    print("image mean %s vs closed form %s: z = %s" % (np.array2string(means.mean(0), precision=6), np.array2string(expected, precision=6), np.array2string(z, precision=2)))
    assert (np.abs(z) <= 5.0).all(), z


def test_importance_does_its_job(ctx):
    rgb = _floor_map()
    expected = E.floor_closed_form(rgb, (1, 1, 1), KD)
    be = _floor()
    e = {}
    for imp in (0, -1):
        _upload(ctx, be, rgb, "y", importance=imp)
        assert ctx.env_info().importance == imp
        film = ctx.render(jp.render_params(32, 32, 256, 1, 99))
        e[imp] = float(np.sqrt(((film.astype(np.float64) - expected[None, None]) ** 2).sum(-1)).mean())
    print("mean per-pixel L2 to the closed form at 256 spp: importance on %.5f, off (uniform solid angle) %.5f, ratio %.3f" % (e[0], e[-1], e[0] / e[-1]))
    assert e[0] <= 0.5 * e[-1], e                                       # the restatement predicts about 0.14 (per-sample relative sd 1.6 against 11.5)


# ---- 5. a constant map against the code that exists ------------------------------------------------------------------------------------------
W = Hh = 48
ENV = (0.3, 0.3, 0.3)


def _l2(film, R):
    """mean per-pixel L2 over the pixels where no channel of either film reaches 0.99 (Clamp01 biases those), and the share left out"""
    keep = (R < 0.99).all(-1) & (film < 0.99).all(-1)
    return float(np.sqrt(((film - R)[keep].astype(np.float64) ** 2).sum(-1)).mean()), 1.0 - keep.mean()


def _statistics(render, R, tag):
    """the statistics of tests/test_gpu_light_pick.py, restated: the error falls as an unbiased estimator's does, and the image mean agrees"""
    assert 1.0 - (R < 0.99).all(-1).mean() <= 0.15
    e = {}
    for spp in (64, 1024):
        e[spp], out = _l2(render(spp, 99), R)
        assert out <= 0.15, (spp, out)
    films = [render(128, 1000 + 17 * k) for k in range(8)]
    keep = (R < 0.99).all(-1)
    for f in films:
        keep &= (f < 0.99).all(-1)
    assert 1.0 - keep.mean() <= 0.15
    means = np.array([f[keep].astype(np.float64).mean() for f in films]); rmean = R[keep].astype(np.float64).mean()
    se = means.std(ddof=1) / np.sqrt(8.0)
    z = (means.mean() - rmean) / se
    print("%s: e(64) = %.5f, e(1024) = %.5f, ratio %.3f; image mean %.6f vs R %.6f, z = %+.2f (left out %.3f)" % (tag, e[64], e[1024], e[1024] / e[64], means.mean(), rmean, z, 1.0 - keep.mean()))
    assert e[1024] <= 0.35 * e[64], e
    assert abs(z) <= 5.0, z


def test_constant_map_is_the_constant_light(ctx):
    be = scenes.build_cornell(scenes.HostBackend("cornell_env"), W, Hh, env=ENV)
    _upload(ctx, be, None)
    R = ctx.render(jp.render_params(W, Hh, 4096, 5, 7))
    assert ctx.light_info().picked_last_render == 1 and ctx.env_info().mapped_last_render == 0 and ctx.env_info().width == 0
    q0, a0, pmf0 = ctx.light_table(); W0 = ctx.light_info().total_weight
    _upload(ctx, be, np.ones((4, 8, 3), f32), "y")
    q1, a1, pmf1 = ctx.light_table(); W1 = ctx.light_info().total_weight
    s = be.flatten().contents
    env = [i for i in range(s.n_lights) if s.light_type[i] == 0]
    assert len(env) == 1
    w0, w1 = float(pmf0[env[0]]) * W0, float(pmf1[env[0]]) * W1
    assert w0 > 0 and abs(w1 - w0) <= 1e-6 * w0 and abs(W1 - W0) <= 1e-6 * W0
    assert np.isclose(w1, E.light_weight(np.ones((4, 8, 3), f32), ENV, s.world_radius), rtol=1e-6)

    def render(spp, seed):
        f = ctx.render(jp.render_params(W, Hh, spp, 5, seed))
        assert ctx.env_info().mapped_last_render == 1
        return f
    _statistics(render, R, "8 x 4 map of ones, tint 0.3, against the constant light")


# ---- 6. plumbing ---------------------------------------------------------------------------------------------------------------------------
def _lit_box(textured=False, env=(0.5, 0.5, 0.5), n_env=1):
    def lamp(be, m):
        scenes.lamp_rect()(be, m)
        for _ in range(n_env):
            be.envlight(env)
    floor = (lambda b: b.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8))) if textured else None
    return scenes.build_lamp_box(scenes.HostBackend("lamp_box_env"), W, Hh, lamp, floor=floor, full_materials=True)


def test_shards_lanes_tone_map_and_textures(ctx):
    rgb = E.bright_map(0.05)
    be = _lit_box()
    _upload(ctx, be, rgb, "y")
    p = lambda **kw: jp.render_params(W, Hh, 8, 5, 1234, **kw)
    whole = ctx.render(p())
    assert whole.mean() > 0.02 and ctx.env_info().mapped_last_render == 1 and ctx.light_info().picked_last_render == 1
    parts = [ctx.render(p(band_rows=5, shard_index=k, shard_count=3)) for k in range(3)]
    assert np.array_equal((parts[0] + parts[1] + parts[2]).view(np.uint32), whole.view(np.uint32))
    assert all((q_ == 0).all(-1).mean() > 0.5 for q_ in parts)
    films = {}
    for lanes in (1, 3):
        ctx.set_options(lanes=lanes)
        films[lanes] = ctx.render(p())
        assert ctx.build_info().lanes_last_render == lanes
    ctx.set_options()
    assert np.array_equal(films[1].view(np.uint32), whole.view(np.uint32)) and np.array_equal(films[3].view(np.uint32), whole.view(np.uint32))
    rgb8, film = ctx.render_rgb8(p(), with_film=True)
    assert np.array_equal(film.view(np.uint32), whole.view(np.uint32))
    enc = np.zeros(film.size, np.uint8)
    jp.host_lib().jp_host_gamma_encode(film.ctypes.data_as(C.c_void_p), film.size, enc.ctypes.data_as(C.c_void_p))
    assert np.array_equal(rgb8.reshape(-1), enc)
    # the fused schedule falls back to the per-bounce launches, and the film is the same
    ctx.set_options(fused=1)
    fused = ctx.render(p())
    assert ctx.build_info().fused_last_render == 0 and ctx.env_info().mapped_last_render == 1
    assert np.array_equal(fused.view(np.uint32), whole.view(np.uint32))
    ctx.set_options()
    # the debug integrator ignores the map, Whitted refuses it
    ctx.render(p(integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))
    assert ctx.env_info().mapped_last_render == 0
    assert ctx.lib.jp_render(ctx.h, C.byref(p(integrator=jp.JP_INTEGRATOR_WHITTED)), film.ctypes.data_as(C.c_void_p)) == -5
    assert b"environment map" in ctx.lib.jp_last_error()
    # the textured twin renders: the checker floor's film differs from the plain one
    bt = _lit_box(textured=True)
    _upload(ctx, bt, rgb, "y", textured=True)
    tex = ctx.render(p())
    assert ctx.texture_info().textured_last_render == 1 and ctx.env_info().mapped_last_render == 1
    assert tex.mean() > 0.02 and not np.array_equal(tex, whole)
    # a different map gives a different film
    _upload(ctx, be, rgb[:, ::-1].copy(), "y")
    assert not np.array_equal(ctx.render(p()), whole)


def test_refusals_and_clearing_the_map(ctx):
    rgb = E.bright_map(0.05)
    be = _lit_box()
    p = jp.render_params(W, Hh, 4, 5, 1234)
    film = np.zeros((Hh, W, 3), f32)
    # a map with JP_LIGHTS_ALL: unsupported; the context stays usable and has no scene, as after any failed upload
    ctx.set_environment_map(rgb, "y"); ctx.set_light_sampling(None)
    assert ctx.lib.jp_upload_scene(ctx.h, be.flatten()) == -5 and b"JP_LIGHTS_POWER_ONE" in ctx.lib.jp_last_error()
    assert ctx.lib.jp_render(ctx.h, C.byref(p), film.ctypes.data_as(C.c_void_p)) == -4
    # two environment lights, and none
    ctx.set_light_sampling("power")
    assert ctx.lib.jp_upload_scene(ctx.h, _lit_box(n_env=2).flatten()) == -1 and b"more than one" in ctx.lib.jp_last_error()
    assert ctx.lib.jp_upload_scene(ctx.h, _lit_box(n_env=0).flatten()) == -1 and b"no JP_LIGHT_ENVIRONMENT" in ctx.lib.jp_last_error()
    assert ctx.lib.jp_render(ctx.h, C.byref(p), film.ctypes.data_as(C.c_void_p)) == -4
    # a bad map is refused when it is set, and the map in force stays
    bad = jp.env_map(rgb); bad.width = 0
    assert ctx.lib.jp_set_environment_map(ctx.h, C.byref(bad)) == -1 and b"size out of range" in ctx.lib.jp_last_error()
    ctx.upload(be.flatten())
    mapped = ctx.render(p)
    assert ctx.env_info().mapped_last_render == 1 and ctx.env_info().width == 16
    assert ctx.lib.jp_env_sample(ctx.h, 1, np.array([0, 0, 0, 0, 1.0], f32).ctypes.data_as(C.c_void_p), None, None, None, None) == -1
    # set_environment_map(None) and a fresh upload: what a context that never saw a map renders
    ctx.set_environment_map(None); ctx.upload(be.flatten())
    cleared = ctx.render(p)
    assert ctx.env_info().mapped_last_render == 0 and ctx.env_info().width == 0 and ctx.env_info().table_bytes_device == 0
    assert ctx.lib.jp_env_lookup(ctx.h, 1, np.array([0, 0, 1.0], f32).ctypes.data_as(C.c_void_p), None, None) == -5
    fresh = jp.Context(0)
    fresh.set_light_sampling("power"); fresh.upload(be.flatten())
    never = fresh.render(p)
    fresh.close()
    assert np.array_equal(cleared.view(np.uint32), never.view(np.uint32)) and not np.array_equal(cleared, mapped)


def test_device_memory_returns():
    start = jp.device_bytes_in_use()
    c = jp.Context(0)
    _upload(c, _lit_box(), E.bright_map(0.05), "y")
    c.render(jp.render_params(W, Hh, 2, 5, 1234))
    held = jp.device_bytes_in_use()
    assert held - start >= c.env_info().table_bytes_device > 0
    c.close()
    assert jp.device_bytes_in_use() == start


def _pfm(path, a):
    a = np.asarray(a, f32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        f.write(a[::-1].astype("<f4").tobytes())


def test_host_api_and_command_line(ctx, tmp_path):
    # FScene::SetEnvironmentMap through the host library's integrator == the C ABI; POWER_ONE is implied
    rgb = E.bright_map(0.05)
    be = _lit_box()
    be.envmap(rgb, "y")
    film = np.zeros((Hh, W, 3), f32); cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    ctx.set_environment_map(be.flatten_envmap()); ctx.set_light_sampling("power"); ctx.upload(be.flatten())
    direct = ctx.render(jp.render_params(W, Hh, 4, 5, 1234))
    assert film.mean() > 0.02 and np.array_equal(film.view(np.uint32), direct.view(np.uint32))
    be.envmap(None)                                                     # ... and without the map again: the scene's own mode, JP_LIGHTS_ALL
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    ctx.set_environment_map(None); ctx.set_light_sampling(None); ctx.upload(be.flatten())
    assert np.array_equal(film.view(np.uint32), ctx.render(jp.render_params(W, Hh, 4, 5, 1234)).view(np.uint32))
    # a mapped scene with no environment light, or two: refused with the library's status
    for n_env in (0, 2):
        bad = _lit_box(n_env=n_env); bad.envmap(rgb, "y")
        assert jp.host_lib().jp_host_render(bad.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == -1
    # jetpbrt --envmap sky.pfm --envmap-up y
    root = scenes.export_reference_layout(str(tmp_path / "scene"), 24, 16)
    sky = str(tmp_path / "sky.pfm"); _pfm(sky, rgb)
    out = str(tmp_path / "cornell")
    args = [jp.CLI_PATH, "0", "8", "64", "48", "--assets", root, "--out", out]
    r = subprocess.run(args + ["--envmap", sky, "--envmap-up", "y"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(open(out + ".bmp", "rb").read()[54:], np.uint8).reshape(48, 64, 3)[::-1, :, ::-1]
    hb = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 48, env=(1.0, 1.0, 1.0))
    p = jp.render_params(64, 48, 8, 5, 1234)
    _upload(ctx, hb, rgb, "y")
    assert np.array_equal(img, ctx.render_rgb8(p))
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    plain = np.frombuffer(open(out + ".bmp", "rb").read()[54:], np.uint8).reshape(48, 64, 3)[::-1, :, ::-1]
    assert not np.array_equal(img, plain)
    open(str(tmp_path / "bad.pfm"), "wb").write(open(sky, "rb").read()[:-7])
    r = subprocess.run(args + ["--envmap", str(tmp_path / "bad.pfm")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 5 and "truncated" in r.stderr
    r = subprocess.run(args + ["--envmap", sky, "--envmap-up", "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 5
