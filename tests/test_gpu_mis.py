"""Multiple importance sampling on the MI355X (INTEGRATION.md "Estimator"): the light strategy's pdf is the definition and the same number on both sides,
the film is the next-event estimator's wherever every weight is 1, the paths are the same paths, the estimator is unbiased against closed forms and
does its job where next-event estimation alone does badly, and the plumbing (shards, lanes, tone map, textures, fused fallback, refusals, memory, host
API, command line) holds.  The restatement is tests/mis_ref.py; the figures these tests print are recorded in DESIGN.md "Estimator"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import envmap_ref as E
import mis_ref as M

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTERS = ("samples", "closest_rays", "closest_hits", "shadow_rays", "shadow_occluded")


@pytest.fixture()
def ctx():
    """a context of its own per test: the estimator, the map and the light sampling mode are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _upload(ctx, be, rgb=None, up="z", mode="power", textured=False):
    ctx.set_environment_map(rgb, up)
    ctx.set_light_sampling(mode)
    ctx.upload(be.flatten(), be.flatten_textures() if textured else None)


def _render(ctx, est, params):
    ctx.set_estimator(est)
    film = ctx.render(params)
    assert ctx.estimator_info().mis_last_render == (1 if est == "mis" else 0)
    c = ctx.counters()
    return film, tuple(getattr(c, k) for k in COUNTERS)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. jp_light_pdf is the definition --------------------------------------------------------------------------------------------------------
TINT = (0.5, 1.0, 0.75)


def _tri_asset():
    p = os.path.join(scenes.asset_dir(), "mis_probe_triangle.obj")
    if not os.path.exists(p):
        scenes.write_obj(p, np.array([(-2.0, -0.6, 0.1), (-1.0, -0.5, -0.2), (-1.6, 0.7, 0.15)], f32), np.array([(0, 1, 2)]))
    return p


def _probe_scene():
    """four emitters near the plane z = 0, spread along x, and an environment light: rectangle, triangle, disk, sphere"""
    be = scenes.HostBackend("mis_probe")
    be.camera((0, 0, 8), (0, 0, -1), (0, 1, 0), 60.0, 16, 16)
    be.envlight(TINT)
    m = be.mat_matte((0.5, 0.5, 0.5))
    be.rect(scenes.AXIS_XY, -4.6, -3.4, -0.5, 0.7, 0.1, False, m, (3.0, 2.0, 1.0))
    be.mesh(_tri_asset(), False, False, mat=m, radiance=(1.0, 4.0, 2.0))
    be.disk((1.5, 0.1, -0.1), scenes._normalize((0.2, -0.3, 1.0)), 0.6, m, (2.0, 2.0, 5.0))
    be.sphere((4.5, 0.0, 0.0), 0.9, m, (6.0, 1.0, 1.0))
    be.preprocess()
    return be


def _probe_rays(shapes, rng, n=2000):
    """origins in two slabs on either side of the emitters (outside every one of them), aimed at points inside the emitters or anywhere"""
    o = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(1.0, 3.0, n) * rng.choice([-1.0, 1.0], n)], -1)
    tgt = np.zeros((n, 3))
    which = rng.integers(0, len(shapes) + 1, n)
    for i, sh in enumerate(shapes):
        k = which == i; c = int(k.sum())
        if sh["kind"] == M.SPHERE:
            v = rng.normal(size=(c, 3)); tgt[k] = sh["c"] + 0.6 * sh["r"] * v / np.linalg.norm(v, axis=-1, keepdims=True)
        elif sh["kind"] == M.DISK:
            v = rng.normal(size=(c, 3)); v -= (v @ sh["n"])[:, None] * sh["n"]
            tgt[k] = sh["c"] + 0.8 * sh["r"] * rng.random((c, 1)) * v / np.linalg.norm(v, axis=-1, keepdims=True)
        elif sh["kind"] == M.RECTANGLE:
            tgt[k] = sh["p1"] + rng.uniform(0.05, 0.95, (c, 1)) * (sh["p0"] - sh["p1"]) + rng.uniform(0.05, 0.95, (c, 1)) * (sh["p2"] - sh["p1"])
        else:
            b = rng.dirichlet((1, 1, 1), c) * 0.85 + 0.05
            tgt[k] = b[:, :1] * sh["p0"] + b[:, 1:2] * sh["p1"] + b[:, 2:] * sh["p2"]
    k = which == len(shapes)
    tgt[k] = o[k] + rng.normal(size=(int(k.sum()), 3))
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    d = (d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)).astype(f32)
    return o.astype(f32), d


@pytest.mark.parametrize("env", [None, "z", "y"])
def test_light_pdf_is_the_definition(ctx, env):
    be = _probe_scene()
    rgb = None
    if env is not None:
        rgb = np.random.default_rng(3).uniform(0.05, 0.95, (2, 4, 3)).astype(f32)
    _upload(ctx, be, rgb, env or "z")
    s = be.flatten().contents
    shapes, lights = M.shapes_of(s), M.lights_of(s)
    assert sorted(sh["kind"] for sh in shapes) == [0, 1, 2, 3] and len(lights) == 5
    _, _, pmf = ctx.light_table()
    assert (pmf > 0).all()
    o, d = _probe_rays(shapes, np.random.default_rng(11))
    light, a = ctx.light_pdf(o, d, 1e-3, 1e30)
    envd = None if env is None else dict(rgb=rgb, tint=TINT, up=E.UP_Z if env == "z" else E.UP_Y)
    rl, ra, cosl, border, cone = M.light_pdf(shapes, lights, pmf, o, d, envd)
    # well-conditioned rays only: |cos| at a flat light >= 0.05 (the division), a texel border no nearer than 1e-3 texels (the lookup's (int)), and a
    # sphere light whose cone has 1 - cos_max >= 0.05 -- sample_li forms that difference in fp32, relative error up to 2^-24 / (1 - cos_max), which a
    # small distant sphere turns into more than the handful of roundings the 1e-5 allows (the same reasoning as for the division)
    keep = (cosl >= 0.05) & (border >= 1e-3) & (cone >= 0.05)
    print("env %s: %d rays, %d kept; lights reached: %s" % (env, len(o), keep.sum(), np.bincount(rl[keep] + 1, minlength=6)))
    assert keep.mean() > 0.8 and (np.bincount(rl[keep] + 1, minlength=6) > 20).all()      # every emitter, the environment and "nothing" (a triangle's back)
    assert np.array_equal(light[keep], rl[keep])
    pos = keep & (ra > 0)
    rel = np.abs(a[pos].astype(np.float64) - ra[pos]) / ra[pos]
    print("env %s: largest relative difference of the pdf: %.3e" % (env, rel.max()))
    assert rel.max() <= 1e-5
    assert (a[keep & (ra == 0)] == 0).all()
    # rays that leave from inside the sphere light
    sp = [sh for sh in shapes if sh["kind"] == M.SPHERE][0]
    v = np.random.default_rng(5).normal(size=(64, 3)); v /= np.linalg.norm(v, axis=-1, keepdims=True)
    li, ai = ctx.light_pdf((sp["c"] + 0.5 * sp["r"] * v[::-1]).astype(f32), v.astype(f32), 1e-3, 1e30)
    assert (ai == 0).all() and (li == -1).all()


# ---- 2. both strategies see the same pdf ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", ["z", "y"])
def test_both_strategies_see_the_same_pdf(ctx, up):
    rgb = E.bright_map()
    be = _probe_scene()
    _upload(ctx, be, rgb, up)
    s = be.flatten().contents
    envl = [i for i in range(s.n_lights) if s.light_type[i] == 0][0]
    _, _, pmf = ctx.light_table()
    rng = np.random.default_rng(17)
    u = np.concatenate([rng.random((1000, 3)), rng.uniform(0.05, 0.95, (1000, 2))], -1).astype(f32)
    idx, wi, Li, pdf = ctx.env_sample(u)
    back, _ = ctx.env_lookup(wi)
    assert np.array_equal(back, idx)                                   # the direction stays inside its texel: no case is left out below
    light, a = ctx.light_pdf(np.zeros((1000, 3), f32), wi, 1e-3, 1e-2)      # (a far end of 0.01: nothing is hit, whatever the direction)
    assert (light == envl).all()
    assert _same(a, (pmf[envl] * pdf).astype(f32))


# ---- 3. where every weight is 1, the film is the next-event estimator's -------------------------------------------------------------------------
W = Hh = 32


def _delta_box():
    def lamp(be, m):
        be.pointlight((278, 273, -200), (630000.0 * 0.2, 650000.0 * 0.2, 650000.0 * 0.2))
        be.dirlight((0.3, -1.0, -0.6), (1.5, 1.2, 0.9))
    return scenes.build_lamp_box(scenes.HostBackend("mis_delta_box"), W, Hh, lamp, full_materials=True)


def _specular_scene():
    be = scenes.HostBackend("mis_specular")
    be.camera((0, 2, 6), scenes._normalize((0, -0.2, -1)), (0, 1, 0), 50.0, W, Hh)
    mirror = be.mat_mirror((0.9, 0.9, 0.9)); glass = be.mat_glass(1.5, (0.98, 0.98, 0.98), (0.98, 0.98, 0.98))
    be.rect(scenes.AXIS_XZ, -1, 1, -1, 1, 4.0, True, mirror, (4.0, 3.0, 2.0))
    be.rect(scenes.AXIS_XZ, -4, 4, -4, 4, 0.0, False, mirror)
    be.rect(scenes.AXIS_XY, -4, 4, 0, 5, -4.0, False, mirror)
    be.sphere((-1.2, 1.0, 0.0), 1.0, glass)
    be.sphere((1.3, 0.8, 0.5), 0.8, mirror)
    be.preprocess()
    return be


@pytest.mark.parametrize("scene", ["delta_lights", "mirror_and_glass"])
def test_film_is_unchanged_where_every_weight_is_one(ctx, scene):
    be = _delta_box() if scene == "delta_lights" else _specular_scene()
    _upload(ctx, be)
    p = jp.render_params(W, Hh, 16, 5, 1234)
    nee, cn = _render(ctx, "nee", p)
    mis, cm = _render(ctx, "mis", p)
    assert nee.mean() > 0.01 and cn[1] > cn[0] > 0
    assert _same(mis, nee) and cm == cn


# ---- 4. same paths ------------------------------------------------------------------------------------------------------------------------------
def _lit_box(textured=False, env=(0.5, 0.5, 0.5)):
    def lamp(be, m):
        scenes.lamp_rect()(be, m)
        be.envlight(env)
        be.sphere((420, 90, -120), 50.0, be.mat_plastic((0.35, 0.12, 0.48), (0.3, 0.25, 0.2), 0.05, False))
    floor = (lambda b: b.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8))) if textured else None
    return scenes.build_lamp_box(scenes.HostBackend("mis_lit_box"), W, Hh, lamp, floor=floor, full_materials=True)


def test_same_paths(ctx):
    _upload(ctx, _lit_box(), E.bright_map(0.05), "y")
    p = jp.render_params(W, Hh, 16, 5, 1234)
    nee, cn = _render(ctx, "nee", p)
    mis, cm = _render(ctx, "mis", p)
    print("counters: %s" % (cn,))
    assert cm == cn and cn[3] > 0 and cn[4] > 0
    assert not _same(mis, nee) and abs(float(mis.mean()) - float(nee.mean())) < 0.05 and np.isfinite(mis).all()


# ---- 5. unbiased against the closed form --------------------------------------------------------------------------------------------------------
KD = (0.8, 0.7, 0.6)


def _floor_under_rect(Le):
    be = scenes.HostBackend("mis_floor_rect")
    be.camera((0, 5, 0), (0, -1, 0), (0, 0, -1), 40.0, W, Hh)
    be.rect(scenes.AXIS_XZ, -50, 50, -50, 50, 0.0, False, be.mat_matte(KD))
    be.rect(scenes.AXIS_XZ, 2.5, 4.5, -1.0, 1.0, 2.0, True, be.mat_matte((0.5, 0.5, 0.5)), Le)      # outside the camera's view, facing the floor
    be.preprocess()
    return be


def _floor_points(cam, sub=4):
    """where the rays through sub x sub positions of every pixel meet the plane y = 0 -> (Hh, W, sub * sub, 3)"""
    pos, fr, ri, up = (np.array(list(v), np.float64) for v in (cam.pos, cam.front, cam.right, cam.up))
    off = (np.arange(sub) + 0.5) / sub
    x = (np.arange(W)[None, :, None, None] + off[None, None, None, :]); y = (np.arange(Hh)[:, None, None, None] + off[None, None, :, None])
    x, y = np.broadcast_arrays(x, y)
    d = fr + ri * (x / W - 0.5)[..., None] + up * (0.5 - y / Hh)[..., None]
    t = -pos[1] / d[..., 1]
    return (pos + t[..., None] * d).reshape(Hh, W, sub * sub, 3)


def _z_scores(films, expected):
    top = max(float(f.max()) for f in films)
    print("largest pixel value of the eight films: %.4f" % top)
    assert top < 0.99                                                   # no pixel clamped (Clamp01 would bias the mean)
    means = np.array([f.astype(np.float64).mean((0, 1)) for f in films])
    se = means.std(0, ddof=1) / np.sqrt(len(films))
    z = (means.mean(0) - expected) / se
    print("image mean %s vs closed form %s: z = %s" % (np.array2string(means.mean(0), precision=6), np.array2string(expected, precision=6), np.array2string(z, precision=2)))
    return z


def test_unbiased_against_the_polygon_formula(ctx):
    Le = np.array([6.0, 5.0, 4.0])
    be = _floor_under_rect(Le)
    _upload(ctx, be)
    s = be.flatten().contents
    lamp = [sh for sh in M.shapes_of(s) if sh["light"] >= 0][0]
    assert lamp["n"][1] < 0                                             # faces the floor
    pts = _floor_points(s.camera)
    irr = M.polygon_irradiance(M.rect_corners(lamp), pts.reshape(-1, 3), np.array([0.0, 1.0, 0.0])).reshape(Hh, W, -1).mean(-1)
    expected = (np.asarray(KD)[None, None] / np.pi * Le[None, None] * irr[..., None]).mean((0, 1))
    ctx.set_estimator("mis")
    films = [ctx.render(jp.render_params(W, Hh, 128, 1, 1000 + 17 * k)) for k in range(8)]
    assert ctx.estimator_info().mis_last_render == 1
    z = _z_scores(films, expected)
    assert (np.abs(z) <= 5.0).all(), z


def test_unbiased_under_the_map(ctx):
    be = scenes.HostBackend("mis_floor_map")
    be.camera((0, 5, 0), (0, -1, 0), (0, 0, -1), 40.0, W, Hh)
    be.envlight((1.0, 1.0, 1.0))
    be.rect(scenes.AXIS_XZ, -50, 50, -50, 50, 0.0, False, be.mat_matte(KD))
    be.preprocess()
    rgb = E.bright_map()
    rgb = (rgb * f32(0.559 / E.floor_closed_form(rgb, (1, 1, 1), KD).max())).astype(f32)
    expected = E.floor_closed_form(rgb, (1, 1, 1), KD)
    _upload(ctx, be, rgb, "y")
    ctx.set_estimator("mis")
    films = [ctx.render(jp.render_params(W, Hh, 128, 1, 1000 + 17 * k)) for k in range(8)]
    assert ctx.estimator_info().mis_last_render == 1 and ctx.env_info().mapped_last_render == 1
    z = _z_scores(films, expected)
    assert (np.abs(z) <= 5.0).all(), z


# ---- 6. MIS does its job ------------------------------------------------------------------------------------------------------------------------
def _rect_facing(be, axis, a0, a1, b0, b1, c, want, mat, radiance):
    """a rectangle light whose normal has a positive dot product with `want`"""
    for flip in (False, True):
        probe = scenes.HostBackend("mis_probe_rect")
        probe.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 4, 4)
        probe.rect(axis, a0, a1, b0, b1, c, flip, probe.mat_matte((0.5, 0.5, 0.5)), (1.0, 1.0, 1.0))
        probe.preprocess()
        n = M.shapes_of(probe.flatten().contents)[0]["n"]
        if n @ np.asarray(want, np.float64) > 0:
            be.rect(axis, a0, a1, b0, b1, c, flip, mat, radiance)
            return
    raise AssertionError("no orientation of the rectangle faces %s" % (want,))


def _lamp_scene():
    L = M.LAMP
    be = scenes.HostBackend("mis_lamp")
    be.camera((0.95 * L["half"], L["height"] / 2, 0), (-1, 0, 0), (0, 1, 0), 40.0, W, Hh)
    be.rect(scenes.AXIS_XZ, -L["half"], L["half"], -L["half"], L["half"], 0.0, False, be.mat_matte((L["kd"],) * 3))
    _rect_facing(be, scenes.AXIS_XZ, -L["half"], L["half"], -L["half"], L["half"], L["height"], (0, -1, 0), be.mat_matte((0.5, 0.5, 0.5)), (L["Le"],) * 3)
    be.preprocess()
    return be


def _metal_scene():
    m = M.METAL
    be = scenes.HostBackend("mis_metal")
    eye = np.array(m["eye"], f32)
    be.camera(eye, scenes._normalize(-eye), (0, 1, 0), 10.0, W, Hh)
    be.rect(scenes.AXIS_XZ, -3, 3, -3, 3, 0.0, False, be.mat_metal(m["eta3"], m["k3"], m["alpha"], m["alpha"], False))
    _rect_facing(be, scenes.AXIS_YZ, m["light_y"][0], m["light_y"][1], m["light_z"][0], m["light_z"][1], m["light_x"], (1, 0, 0), be.mat_matte((0.5, 0.5, 0.5)), (m["Le"],) * 3)
    be.preprocess()
    return be


def _converse_scene():
    be = scenes.HostBackend("mis_converse")
    be.camera((0, 5, 0), (0, -1, 0), (0, 0, -1), 40.0, W, Hh)
    be.rect(scenes.AXIS_XZ, -50, 50, -50, 50, 0.0, False, be.mat_matte((0.8, 0.8, 0.8)))
    _rect_facing(be, scenes.AXIS_XZ, 3.0, 3.1, -0.05, 0.05, 6.0, (0, -1, 0), be.mat_matte((0.5, 0.5, 0.5)), (2000.0,) * 3)
    be.preprocess()
    return be


def _variance_ratio(ctx, be):
    """empirical per-pixel variance (first channel) over eight seeds at 64 spp, averaged over the pixels whose centre sees the floor (primitive 0): MIS / NEE"""
    _upload(ctx, be)
    cam = be.flatten().contents.camera
    pos, fr, ri, up = (np.array(list(v), np.float64) for v in (cam.pos, cam.front, cam.right, cam.up))
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(Hh) + 0.5)
    d = fr + ri * (x / W - 0.5)[..., None] + up * (0.5 - y / Hh)[..., None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(f32)
    hit, _, prim, _ = ctx.trace(np.tile(pos.astype(f32), (W * Hh, 1)), d, np.full(W * Hh, 1e-3, f32), np.full(W * Hh, 1e30, f32))
    floor = ((hit != 0) & (prim == 0)).reshape(Hh, W)
    assert floor.sum() >= 200
    var = {}
    for est in ("nee", "mis"):
        ctx.set_estimator(est)
        films = np.array([ctx.render(jp.render_params(W, Hh, 64, 1, 500 + 31 * k))[..., 0] for k in range(8)], np.float64)
        var[est] = float(films.var(0, ddof=1)[floor].mean())
        print("  %s: largest floor pixel %.3f, mean %.4f, mean per-pixel variance %.3e" % (est, films[:, floor].max(), films[:, floor].mean(), var[est]))
    return var["mis"] / var["nee"]


@pytest.mark.parametrize("scene", ["lamp", "metal"])
def test_mis_does_its_job(ctx, scene):
    pred = M.lamp_prediction() if scene == "lamp" else M.metal_prediction()
    predicted = pred["mis"][1] / pred["nee"][1]
    bound = float(np.sqrt(predicted))                                   # halfway, on a log scale, between the prediction and "no gain"
    measured = _variance_ratio(ctx, _lamp_scene() if scene == "lamp" else _metal_scene())
    print("%s: variance MIS / NEE predicted %.3e, bound %.3e, measured %.3e" % (scene, predicted, bound, measured))
    assert measured <= bound


def test_converse_scene_is_recorded(ctx):
    # a small distant light on matte: next-event estimation is the good strategy here; the ratio is recorded (DESIGN.md "Estimator"), nothing is asserted about it
    measured = _variance_ratio(ctx, _converse_scene())
    print("converse (small distant light on matte): variance MIS / NEE measured %.3f" % measured)
    assert np.isfinite(measured)


# ---- 7. plumbing ----------------------------------------------------------------------------------------------------------------------------------
def test_shards_lanes_tone_map_textures_and_refusals(ctx):
    rgb = E.bright_map(0.05)
    be = _lit_box()
    _upload(ctx, be, rgb, "y")
    ctx.set_estimator("mis")
    p = lambda **kw: jp.render_params(W, Hh, 8, 5, 1234, **kw)
    whole = ctx.render(p())
    info = ctx.estimator_info()
    assert whole.mean() > 0.02 and info.mode == jp.JP_ESTIMATOR_MIS and info.mis_last_render == 1 and info.side_bytes_device > 0
    assert ctx.env_info().mapped_last_render == 1 and ctx.light_info().picked_last_render == 1
    parts = [ctx.render(p(band_rows=5, shard_index=k, shard_count=2)) for k in range(2)]
    assert _same(parts[0] + parts[1], whole) and all((q_ == 0).all(-1).mean() > 0.3 for q_ in parts)
    films = {}
    for lanes in (1, 3):
        ctx.set_options(lanes=lanes)
        films[lanes] = ctx.render(p())
        assert ctx.build_info().lanes_last_render == lanes and ctx.estimator_info().mis_last_render == 1
    ctx.set_options()
    assert _same(films[1], whole) and _same(films[3], whole)
    rgb8, film = ctx.render_rgb8(p(), with_film=True)
    assert _same(film, whole)
    enc = np.zeros(film.size, np.uint8)
    jp.host_lib().jp_host_gamma_encode(film.ctypes.data_as(C.c_void_p), film.size, enc.ctypes.data_as(C.c_void_p))
    assert np.array_equal(rgb8.reshape(-1), enc)
    # the fused schedule falls back to the per-bounce launches, and the film is the same
    ctx.set_options(fused=1)
    fused = ctx.render(p())
    assert ctx.build_info().fused_last_render == 0 and ctx.estimator_info().mis_last_render == 1 and _same(fused, whole)
    ctx.set_options()
    # the debug integrator ignores the estimator, Whitted refuses it; the context stays usable
    ctx.render(p(integrator=jp.JP_INTEGRATOR_DEBUG_NORMAL))
    assert ctx.estimator_info().mis_last_render == 0
    assert ctx.lib.jp_render(ctx.h, C.byref(p(integrator=jp.JP_INTEGRATOR_WHITTED)), film.ctypes.data_as(C.c_void_p)) == -5
    assert _same(ctx.render(p()), whole)
    # a bad mode is refused and the mode in force stays
    bad = jp.JpEstimator(C.sizeof(jp.JpEstimator), 7)
    assert ctx.lib.jp_set_estimator(ctx.h, C.byref(bad)) == -1 and ctx.estimator_info().mode == jp.JP_ESTIMATOR_MIS
    # without the map: the pick family
    _upload(ctx, be)
    nomap = ctx.render(p())
    assert ctx.estimator_info().mis_last_render == 1 and ctx.env_info().mapped_last_render == 0 and not _same(nomap, whole)
    # the textured twin renders: the checker floor's film differs from the plain one
    _upload(ctx, _lit_box(textured=True), rgb, "y", textured=True)
    tex = ctx.render(p())
    assert ctx.texture_info().textured_last_render == 1 and ctx.estimator_info().mis_last_render == 1
    assert tex.mean() > 0.02 and not _same(tex, whole)
    # jp_set_estimator(NULL): back to next-event estimation, the film of a context that never heard of the estimator
    _upload(ctx, be, rgb, "y")
    ctx.set_estimator(None)
    back = ctx.render(p())
    assert ctx.estimator_info().mis_last_render == 0 and ctx.estimator_info().mode == jp.JP_ESTIMATOR_NEE
    fresh = jp.Context(0)
    _upload(fresh, be, rgb, "y")
    never = fresh.render(p())
    fresh.close()
    assert _same(back, never) and not _same(back, whole)


def test_a_scene_without_the_light_table_is_refused_at_render(ctx):
    be = _lit_box()
    _upload(ctx, be, None, mode=None)                                    # JP_LIGHTS_ALL
    p = jp.render_params(W, Hh, 4, 5, 1234)
    nee = ctx.render(p)
    ctx.set_estimator("mis")
    film = np.zeros((Hh, W, 3), f32)
    assert ctx.lib.jp_render(ctx.h, C.byref(p), film.ctypes.data_as(C.c_void_p)) == -5 and b"JP_LIGHTS_POWER_ONE" in ctx.lib.jp_last_error()
    assert ctx.lib.jp_light_pdf(ctx.h, 1, *[np.zeros(3, f32).ctypes.data_as(C.c_void_p)] * 6) == -5
    assert ctx.estimator_info().side_bytes_device == 0
    ctx.set_estimator("nee")
    assert _same(ctx.render(p), nee)


# ---- 8. device memory -------------------------------------------------------------------------------------------------------------------------------
def test_device_memory_returns():
    start = jp.device_bytes_in_use()
    c = jp.Context(0)
    _upload(c, _lit_box(), E.bright_map(0.05), "y")
    p = jp.render_params(W, Hh, 2, 5, 1234)
    c.render(p)
    assert c.estimator_info().side_bytes_device == 0
    before = jp.device_bytes_in_use()
    c.set_estimator("mis")
    c.render(p)
    side = c.estimator_info().side_bytes_device
    assert side > 0 and jp.device_bytes_in_use() - before >= side
    c.close()
    assert jp.device_bytes_in_use() == start


# ---- 9. host API and command line -------------------------------------------------------------------------------------------------------------------
def test_host_api_and_command_line(ctx, tmp_path):
    # FScene::SetEstimator through the host library's integrator == the C ABI; POWER_ONE is implied
    be = _lit_box()
    be.set_estimator("mis")
    film = np.zeros((Hh, W, 3), f32); cnt = jp.JpCounters()
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    _upload(ctx, be)
    p = jp.render_params(W, Hh, 4, 5, 1234)
    direct, _ = _render(ctx, "mis", p)
    nee, _ = _render(ctx, "nee", p)
    assert film.mean() > 0.02 and _same(film, direct) and not _same(film, nee)
    be.set_estimator(None)                                              # ... and back: the scene's own mode, JP_LIGHTS_ALL
    assert jp.host_lib().jp_host_render(be.h, W, Hh, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
    _upload(ctx, be, None, mode=None)
    assert _same(film, ctx.render(p))
    # jetpbrt --estimator mis
    root = scenes.export_reference_layout(str(tmp_path / "scene"), 24, 16)
    out = str(tmp_path / "cornell")
    args = [jp.CLI_PATH, "0", "8", "64", "48", "--assets", root, "--out", out]
    r = subprocess.run(args + ["--estimator", "mis"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(open(out + ".bmp", "rb").read()[54:], np.uint8).reshape(48, 64, 3)[::-1, :, ::-1]
    hb = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 48)
    _upload(ctx, hb)
    ctx.set_estimator("mis")
    assert np.array_equal(img, ctx.render_rgb8(jp.render_params(64, 48, 8, 5, 1234)))
    ctx.set_estimator("nee")
    assert not np.array_equal(img, ctx.render_rgb8(jp.render_params(64, 48, 8, 5, 1234)))
