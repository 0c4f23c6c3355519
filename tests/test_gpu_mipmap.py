"""Mip maps on the MI355X (INTEGRATION.md "Mip maps"): the uploaded pyramid against the host builder, jp_mip_probe -- the device function k_texel_m calls -- bit for
bit against the host functions and the numpy restatement on the four shapes, the no-op rule, three films that are bit-identical to a constant image's by
construction (direct view, a width carried across a mirror, a spread widened by a diffuse bounce; lanes and reused slots), the albedo guide, the refusals at upload,
and the schedule's rules for textured scenes."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import mipmap_ref as M
import tex_sampling_ref as TR

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARGUMENT = -1
RP = jp.JP_WRAP_REPEAT
IMG64 = np.random.default_rng(17).integers(0, 256, (64, 64, 3), dtype=np.uint8)
IMG53 = np.random.default_rng(18).integers(0, 256, (3, 5, 3), dtype=np.uint8)
GREY = np.full((1, 1, 3), 128, np.uint8)


def _checker(n, cell):
    i = np.arange(n) // cell
    c = (((i[:, None] + i[None, :]) & 1) * 255).astype(np.uint8)
    return np.repeat(c[:, :, None], 3, 2)


@pytest.fixture()
def ctx():
    """a context of its own per test: the mipmap modes and the sampling records are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _upload(ctx, be, mip=None, **kw):
    """the scene's sampling records, its mipmap modes (None: no state; a list of modes else), then the textured upload"""
    ctx.set_texture_sampling(be.flatten_texture_sampling())
    ctx.set_texture_mipmaps(None if mip is None else jp.texture_mipmaps(mip, **kw))
    ctx.upload(be.flatten(), be.flatten_textures())


def _render(ctx, W, H, spp, depth, **kw):
    return ctx.render(jp.render_params(W, H, spp, depth, 1234, **kw))


def _camera_dirs(cam, xs, ys):
    """directions of the camera rays through film positions (xs, ys), as k_raygen forms them"""
    front, right, up = (np.array(getattr(cam, k), f32) for k in ("front", "right", "up"))
    X, Y = np.meshgrid(np.asarray(xs, f32), np.asarray(ys, f32))
    d = front + right * (X.ravel()[:, None] / f32(cam.res_x) - f32(0.5)) + up * (f32(0.5) - Y.ravel()[:, None] / f32(cam.res_y))
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------------------------------------
def test_uploaded_pyramid_equals_the_host_builder(ctx):
    be = scenes.HostBackend("mip_chain")
    be.camera((0, 0, 50), (0, 0, -1), (0, 1, 0), 60.0, 8, 8)
    be.envlight((1, 1, 1))
    be.rect(scenes.AXIS_XY, -10, 0, -8, 9, -5, False, be.mat_matte(tex=be.texture_image(IMG53)), None)
    be.rect(scenes.AXIS_XY, 0, 10, -8, 9, -5, False, be.mat_matte(tex=be.texture_image(IMG64)), None)
    be.preprocess()
    before = jp.device_bytes_in_use()
    _upload(ctx, be)
    plain = jp.device_bytes_in_use() - before
    _upload(ctx, be, [1, 1])
    i = ctx.texture_mipmap_info()
    higher = sum(w * h for w, h in M.level_sizes(5, 3)[1:] + M.level_sizes(64, 64)[1:])
    assert (i.n_on, i.n_levels, i.mip_last_render, i.cone_bytes_device) == (2, 3 + 7, 0, 0)
    assert i.pyramid_bytes_device == 4 * higher + 2 * 8 + 10 * 16 and i.build_ms >= 0
    assert jp.device_bytes_in_use() - before >= plain + 4 * higher
    for k, img in enumerate((IMG53, IMG64)):
        got = ctx.read_mip_chain(k, img.shape[1], img.shape[0]); want = jp.build_mip_chain(img)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), k
    _upload(ctx, be, [0, 1])
    assert ctx.texture_mipmap_info().n_on == 1
    with pytest.raises(jp.JetPbrtError, match="texture 0 has no pyramid"):
        ctx.read_mip_chain(0, 5, 3)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.read_mip_chain(1, 64, 64), M.build_chain(IMG64)))


# ---- 2. the probe on the four shapes -------------------------------------------------------------------------------------------------------------------------
TRI = np.array([(-12, -10, -2), (13, -9, 1), (0, 12, -1)], f32)
TRI_UV = {"tri": np.array([(0, 0), (3, 0), (1.5, 3)], f32), "tri_degenerate": np.array([(0.3, 0.3), (0.3, 0.3), (0.3, 0.3)], f32)}
SPHERE = ((1, -2, 0), 9.0)
DISK = ((0, 0, -2), (0.2, 0.4, 1.0), 10.0)
RECT = (-10, 12, -8, 9, -5)


def _shape_scene(tmp_path, kind, sampling):
    be = scenes.HostBackend("mip_shapes")
    be.camera((0, 0, 50), (0, 0, -1), (0, 1, 0), 60.0, 4096, 4096)      # (nothing is rendered: the resolution sets gamma0, a camera ray's footprint below a texel)
    be.envlight((0, 0, 0))
    m = be.mat_matte(tex=be.texture_image(IMG64, sampling=sampling))
    if kind == "rect":
        be.rect(scenes.AXIS_XY, RECT[0], RECT[1], RECT[2], RECT[3], RECT[4], False, m, None)
    elif kind in TRI_UV:
        be.mesh(scenes.write_obj(str(tmp_path / (kind + ".obj")), TRI, np.array([(0, 1, 2)]), uvs=TRI_UV[kind]), False, False, mat=m)
    elif kind == "sphere":
        be.sphere(SPHERE[0], SPHERE[1], m, None)
    else:
        be.disk(DISK[0], DISK[1], DISK[2], m, None)
    be.preprocess()
    return be


def _area(kind, p):
    n = len(p)
    if kind == "rect":
        a0, a1, b0, b1, c = RECT
        return M.area_rectangle(np.tile(f32([a0, b0, c]), (n, 1)), np.tile(f32([a1, b0, c]), (n, 1)), np.tile(f32([a0, b1, c]), (n, 1)))
    if kind in TRI_UV:
        return M.area_triangle(np.tile(TRI[0], (n, 1)), np.tile(TRI[1], (n, 1)), np.tile(TRI[2], (n, 1)), np.tile(TRI_UV[kind].reshape(6), (n, 1)))
    if kind == "sphere":
        return M.area_sphere((p - f32(SPHERE[0])).astype(f32), SPHERE[1])
    return M.area_disk((p - f32(DISK[0])).astype(f32), DISK[2])


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)).astype(f32); o[:, 2] += f32(40)
    tgt = rng.uniform(-12, 12, (n, 3)).astype(f32)
    d = (tgt - o).astype(f32)
    d = (d / np.sqrt(_dot(d, d))[:, None]).astype(f32)
    return o, d, np.full(n, 1e-3, f32), np.full(n, np.inf, f32)


@pytest.mark.parametrize("kind", ["rect", "tri", "sphere", "disk", "tri_degenerate"])
def test_probe_equals_the_host_functions_bit_for_bit(ctx, tmp_path, kind):
    """state, rho and colour of jp_mip_probe against jp_mip_cone_step / jp_mip_footprint / jp_texture_lookup_mip and the numpy restatement, without a record and under
    a tiling bilinear record, for bounce 0, bounce 1 specular and bounce 1 diffuse with random incoming states"""
    n = 2048
    rays = _rays(n, 5)
    rng = np.random.default_rng(6)
    flags = np.array([0, 1 | 0x100, 1, 2 | (5 << 16)], np.int32)[rng.integers(0, 4, n)]
    st_in = np.stack([10.0 ** rng.uniform(-2.5, 0, n), rng.uniform(0, 0.0004, n)], -1).astype(f32)      # widths over 2.5 decades: footprints below a texel and levels 0 .. 5
    bs, fs = f32(0.0002), f32(1.5)
    for rec in (None, (RP, RP, jp.JP_FILTER_BILINEAR, (2.0, 3.0), (0.25, 0.5))):
        be = _shape_scene(tmp_path, kind, None if rec is None else jp.tex_sampler(*rec))
        _upload(ctx, be, [1], footprint_scale=fs, bounce_spread=bs)
        info = ctx.texture_mipmap_info()
        cam = be.flatten().contents.camera
        g0 = M.gamma0(cam.up, cam.res_y)
        assert info.n_on == 1 and f32(info.gamma0) == g0 and f32(info.bounce_spread) == bs and f32(info.footprint_scale) == fs
        hit, t, _, _ = ctx.trace(*rays)
        prim0, uv, _ = ctx.surface(*rays)
        st, prim, rho, rgb = ctx.mip_probe(*rays, flags, st_in)
        k = prim >= 0
        assert np.array_equal(prim, prim0) and np.array_equal(k, hit != 0) and k.sum() >= 500
        want_st = jp.mip_cone_step(g0, bs, flags[k], t[k], st_in[k])
        assert _same(want_st, M.cone_step(g0, bs, flags[k], t[k], st_in[k]))
        assert _same(st[k], want_st) and _same(st[~k], st_in[~k])
        p = (rays[0][k] + (t[k][:, None] * rays[1][k]).astype(f32)).astype(f32)
        sc = (1.0, 1.0) if rec is None else rec[3]
        area = _area(kind, p)
        want_rho = jp.mip_footprint(want_st[:, 0], area, 64, 64, sc, fs)
        assert _same(want_rho, M.rho(want_st[:, 0], area, 64, 64, sc, fs))
        assert _same(rho[k], want_rho) and (rho[~k] == 0).all(), (kind, rec, int((rho[k] != want_rho).sum()))
        if kind == "tri_degenerate":
            assert (rho == 0).all()
        else:
            assert (rho[k] > 2).sum() >= 20 and ((rho[k] > 1) & (rho[k] < 2)).sum() >= 20 and (rho[k] <= 1).sum() >= 20, np.percentile(rho[k], [5, 50, 95])
        s_host = None if rec is None else jp.tex_sampler(*rec)
        want_rgb = jp.texture_lookup_mip(s_host, IMG64, uv[k], want_rho)
        assert np.array_equal(want_rgb, M.lookup(None if rec is None else TR.Sampler(*rec), IMG64, uv[k], want_rho))
        assert np.array_equal(rgb[k], want_rgb) and (rgb[~k] == 0).all(), (kind, rec, int((rgb[k] != want_rgb).any(1).sum()))
        low = want_rho <= 1
        assert np.array_equal(rgb[k][low], jp.texture_lookup(s_host, IMG64, uv[k][low]))


# ---- 3. the no-op rule ---------------------------------------------------------------------------------------------------------------------------------------
def _close_wall(img):
    """one wall of one 8 x 8 image 5 units from the camera: a texel is many pixels wide; nothing else, so every textured hit is a camera ray's"""
    be = scenes.HostBackend("mip_close")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 16, 16)
    be.envlight((1, 1, 1))
    be.rect(scenes.AXIS_XY, -10, 10, -10, 10, 0, False, be.mat_matte(tex=be.texture_image(img)), None)
    be.preprocess()
    return be


def test_no_op_rule(ctx):
    img = IMG64[:8, :8]
    be = _close_wall(img)
    before = jp.device_bytes_in_use()
    _upload(ctx, be)
    bytes_plain = jp.device_bytes_in_use() - before
    film0 = _render(ctx, 16, 16, 4, 3); guides0 = ctx.render_guides(jp.render_params(16, 16, 4, 3), 2)
    bytes_rendered = jp.device_bytes_in_use() - before
    assert ctx.texture_mipmap_info().mip_last_render == 0 and film0.std() > 0.01
    # all modes OFF: the upload without the state
    _upload(ctx, be, [0], footprint_scale=2.0, bounce_spread=0.5)
    film1 = _render(ctx, 16, 16, 4, 3); guides1 = ctx.render_guides(jp.render_params(16, 16, 4, 3), 2)
    i = ctx.texture_mipmap_info()
    assert (i.n_on, i.n_levels, i.pyramid_bytes_device, i.cone_bytes_device, i.mip_last_render) == (0, 0, 0, 0, 0)
    assert _same(film0, film1) and all(_same(a, b) for a, b in zip(guides0, guides1)) and jp.device_bytes_in_use() - before <= bytes_rendered
    # mipmaps on, every reachable rho <= 1: k_texel_m runs and writes the words k_texel writes
    _upload(ctx, be, [1], footprint_scale=1.0, bounce_spread=0.01)
    cam = be.flatten().contents.camera
    g0 = M.gamma0(cam.up, cam.res_y)
    d = _camera_dirs(cam, np.arange(0, 16.5, 0.5), np.arange(0, 16.5, 0.5))
    t = (f32(5) / -d[:, 2]).astype(f32)
    rho = M.rho((g0 * t * f32(1.01)).astype(f32), np.full(len(t), 400, f32), 8, 8)
    assert rho.max() <= 0.5                                             # (the wall is the only surface: no later bounce reaches a texture)
    film2 = _render(ctx, 16, 16, 4, 3); guides2 = ctx.render_guides(jp.render_params(16, 16, 4, 3), 2)
    i = ctx.texture_mipmap_info()
    assert (i.n_on, i.mip_last_render) == (1, 1) and i.cone_bytes_device >= 8 * 256 and i.pyramid_bytes_device > 0
    assert _same(film0, film2) and all(_same(a, b) for a, b in zip(guides0, guides2))
    # mipmaps on a texture no material uses: the upload without them
    t = be.flatten_textures().contents
    for m in range(t.n_materials):
        t.mat_texture[m] = -1                                           # (the flattened view, until the next preprocess: the image stays, no material refers to it)
    films = []
    for mip in (None, [1]):
        _upload(ctx, be, mip)
        films.append(_render(ctx, 16, 16, 4, 3))
        i = ctx.texture_mipmap_info()
        assert (i.n_on, i.pyramid_bytes_device, i.cone_bytes_device, i.mip_last_render) == (0, 0, 0, 0) and ctx.texture_info().textured_last_render == 0
    assert _same(films[0], films[1]) and not _same(films[0], film0)
    assert bytes_plain > 0


# ---- 4. exact films ------------------------------------------------------------------------------------------------------------------------------------------
W = H = 16


def _scene_direct(img, scale):
    """a tiled wall facing the camera 30 units away, a lamp behind the camera"""
    be = scenes.HostBackend("mip_direct")
    be.camera((0, 0, 30), (0, 0, -1), (0, 1, 0), 30.0, W, H)
    be.envlight((0, 0, 0))
    be.rect(scenes.AXIS_XY, -10, 10, -10, 10, 0, False, be.mat_matte(tex=be.texture_image(img, sampling=jp.tex_sampler(RP, RP, jp.JP_FILTER_DEFAULT, (scale, scale)))), None)
    be.sphere((0, 0, 45), 3.0, be.mat_matte((0.5, 0.5, 0.5)), (20, 20, 20))
    be.preprocess()
    return be


def _scene_mirror(img, scale):
    """the camera looks down -z at a mirror disk 40 units away, tilted 45 degrees; the textured wall stands 5 units beside the mirror (the plane x = 5) and is seen
    through it alone"""
    be = scenes.HostBackend("mip_mirror")
    be.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 8.0, W, H)
    be.envlight((1, 1, 1))
    be.disk((0, 0, -40), (1, 0, 1), 6.0, be.mat_mirror((1, 1, 1)), None)
    be.rect(scenes.AXIS_YZ, -20, 20, -60, -20, 5, False, be.mat_matte(tex=be.texture_image(img, sampling=jp.tex_sampler(RP, RP, jp.JP_FILTER_DEFAULT, (scale, scale)))), None)
    be.preprocess()
    return be


def _scene_matte(img, scale):
    """the camera looks down -z at a matte floor 20 units away; the textured wall is the plane z = 10 behind the camera, lit by a point light between the two"""
    be = scenes.HostBackend("mip_matte")
    be.camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 20.0, W, H)
    be.envlight((0, 0, 0))
    be.pointlight((3, 2, -5), (400, 400, 400))
    be.rect(scenes.AXIS_XY, -100, 100, -100, 100, -20, False, be.mat_matte((0.8, 0.8, 0.8)), None)
    be.rect(scenes.AXIS_XY, -100, 100, -100, 100, 10, False, be.mat_matte(tex=be.texture_image(img, sampling=jp.tex_sampler(RP, RP, jp.JP_FILTER_DEFAULT, (scale, scale)))), None)
    be.preprocess()
    return be


def _gamma0(be):
    cam = be.flatten().contents.camera
    return M.gamma0(cam.up, cam.res_y), cam


def _films(ctx, build, img, scale, spp=4, depth=4, **kw):
    """(the image with mipmaps, the image without, the 1 x 1 image of byte 128 without) rendered alike"""
    out = []
    for im, mip in ((img, [1]), (img, None), (GREY, None)):
        be = build(im, scale)
        _upload(ctx, be, mip, **kw)
        out.append(_render(ctx, W, H, spp, depth))
        assert ctx.texture_mipmap_info().mip_last_render == (1 if mip else 0)
    assert not _same(out[1], out[2]) and np.abs(out[1] - out[2]).max() > 0.02        # without mipmaps the checker shows: the equality below is the pyramid's doing
    return out


def test_exact_film_direct_view(ctx):
    """the 1-texel checker tiled 4 x 4 over the wall; every camera ray has rho >= 2, and a later hit of the wall has a longer path behind it (width >= gamma0 * path
    length >= gamma0 * the camera's distance from the wall's plane): every level >= 1 is 128"""
    be = _scene_direct(_checker(64, 1), 4.0)
    g0, cam = _gamma0(be)
    d = _camera_dirs(cam, np.arange(0, W + 0.5, 0.5), np.arange(0, H + 0.5, 0.5))
    assert (np.abs(d[:, :2] * (30 / -d[:, 2:3])) < 10).all()             # every camera ray meets the wall
    rho = M.rho((g0 * f32(30)).astype(f32) * np.ones(1, f32), np.full(1, 400, f32), 64, 64, (4.0, 4.0))      # the shortest path to the wall's plane
    assert rho[0] >= 2
    a, _, c = _films(ctx, _scene_direct, _checker(64, 1), 4.0, bounce_spread=0.125)
    assert _same(a, c) and a.mean() > 0.01
    # ... and the albedo guide follows the mip at the first hit
    ga = None
    for im, mip in ((_checker(64, 1), [1]), (GREY, None)):
        _upload(ctx, _scene_direct(im, 4.0), mip, bounce_spread=0.125)
        g = ctx.render_guides(jp.render_params(W, H, 4, 4), 2)
        if ga is None:
            ga = g
    assert all(_same(x, y) for x, y in zip(ga, g)) and _same(ga[0], np.full((H, W, 3), f32(1.0) / f32(255.0) * f32(128), f32))
    _upload(ctx, _scene_direct(_checker(64, 1), 4.0), None)
    assert not _same(ctx.render_guides(jp.render_params(W, H, 4, 4), 2)[0], ga[0])


def _mirror_precondition(be):
    """rho over the camera rays of the mirror scene: (from the whole path, from the last segment alone); the wall is the plane x = 5, the mirror the plane x + z = -40"""
    g0, cam = _gamma0(be)
    d = _camera_dirs(cam, np.arange(0, W + 0.5, 0.5), np.arange(0, H + 0.5, 0.5)).astype(np.float64)
    t1 = -40.0 / (d[:, 0] + d[:, 2])
    p = d * t1[:, None]
    assert (np.linalg.norm(p - np.array([0, 0, -40.0]), axis=1) < 6).all()            # every camera ray meets the mirror
    n = np.array([1, 0, 1.0]) / np.sqrt(2.0)
    r = d - 2 * (d @ n)[:, None] * n
    t2 = (5.0 - p[:, 0]) / r[:, 0]
    q = p + r * t2[:, None]
    assert (r[:, 0] > 0.9).all() and (np.abs(q[:, 1]) < 20).all() and (q[:, 2] > -60).all() and (q[:, 2] < -20).all()   # ... and its reflection the wall
    K = dict(area=np.full(len(d), 1600, f32), w=64, h=64, scale=(8.0, 8.0))
    whole = M.rho((g0 * (t1 + t2).astype(f32) * f32(0.999)).astype(f32), **K)
    last = M.rho((g0 * t2.astype(f32) * f32(1.001)).astype(f32), **K)
    return whole, last


@pytest.mark.parametrize("schedule", ["plain", "lanes2", "reused_slots"])
def test_exact_film_width_carried_across_the_mirror(ctx, schedule):
    """the 2 x 2-cell checker (level 1 is a checker still, levels >= 2 are 128) tiled 8 x 8: rho of the whole path >= 4, of the mirror-to-wall segment alone < 1 --
    a kernel that loses the slot's state between bounces reads level 0 and shows the checker.  The width never shrinks along a path, so every later hit of the wall
    is >= 4 as well, whatever the spread.  Two lanes, and batches that reuse the slots, give the same film."""
    whole, last = _mirror_precondition(_scene_mirror(_checker(64, 2), 8.0))
    assert whole.min() >= 4 and last.max() < 1
    if schedule == "lanes2":
        ctx.set_options(lanes=2, lane_rows=4)
    elif schedule == "reused_slots":
        ctx.set_options(max_slots=W * H)                                # one sample per pixel and batch: four batches through the same 256 slots
    a, _, c = _films(ctx, _scene_mirror, _checker(64, 2), 8.0, bounce_spread=1.0)
    assert _same(a, c) and a.mean() > 0.01
    be = _scene_mirror(_checker(64, 2), 8.0)
    _upload(ctx, be, [1], bounce_spread=1.0)
    _render(ctx, W, H, 4, 4)
    i = ctx.texture_mipmap_info(); lanes = ctx.build_info().lanes_last_render
    assert lanes == (2 if schedule == "lanes2" else 1) and i.cone_bytes_device >= 8 * W * H // (4 if schedule == "reused_slots" else 1)
    if schedule == "lanes2":
        assert i.cone_bytes_device >= 2 * 8 * (W * H // 2) * 4


def test_exact_film_spread_widened_by_a_diffuse_bounce(ctx):
    """camera -> matte floor -> textured wall: with gamma0 alone the perpendicular bounce has rho < 4, with bounce_spread 0.5 every hit of the wall has rho >= 4
    (the camera ray is >= 20 long, the bounce >= 30)"""
    be = _scene_matte(_checker(64, 2), 4.0)
    g0, cam = _gamma0(be)
    K = dict(area=np.full(1, 40000, f32), w=64, h=64, scale=(4.0, 4.0))
    alone = M.rho((g0 * f32(20.3 + 30)).astype(f32) * np.ones(1, f32), **K)            # (20.3: the longest camera ray of the frame)
    widened = M.rho(((g0 * f32(20)).astype(f32) + f32(0.5) * f32(30)).astype(f32) * np.ones(1, f32), **K)
    d = _camera_dirs(cam, [0, W], [0, H])
    assert (20 / -d[:, 2]).max() < 20.3 and alone[0] < 4 and widened[0] >= 4
    a, _, c = _films(ctx, _scene_matte, _checker(64, 2), 4.0, bounce_spread=0.5)
    assert _same(a, c) and a.mean() > 0.01
    # the spread is what does it: with a bounce_spread of gamma0's size the wall's checker reaches the film
    _upload(ctx, _scene_matte(_checker(64, 2), 4.0), [1], bounce_spread=float(g0))
    assert not _same(_render(ctx, W, H, 4, 4), c)


# ---- 5. refusals at the upload ---------------------------------------------------------------------------------------------------------------------------------
def test_upload_refusals_keep_the_scene(ctx):
    be = _close_wall(IMG64[:8, :8])
    _upload(ctx, be, [1])
    want = _render(ctx, 16, 16, 2, 2)

    def check(word):
        assert _same(_render(ctx, 16, 16, 2, 2), want), word
        assert ctx.texture_mipmap_info().n_on == 1, word
    ctx.set_texture_mipmaps(jp.texture_mipmaps([1, 0]))
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.upload(be.flatten(), be.flatten_textures())
    assert "status %d" % INVALID_ARGUMENT in str(e.value) and "n_textures (2)" in str(e.value) and "(1)" in str(e.value) and "jp_set_texture_mipmaps" in str(e.value)
    check("after a refused textured upload")
    with pytest.raises(jp.JetPbrtError, match="n_textures"):
        ctx.upload(be.flatten())
    check("after a refused plain upload")
    with pytest.raises(jp.JetPbrtError, match="unknown mode"):
        ctx.set_texture_mipmaps(jp.texture_mipmaps([7]))
    ctx.set_texture_mipmaps(jp.texture_mipmaps([1]))                     # (the refused state left the old one: this one fits again)
    chk = scenes.HostBackend("mip_checker")
    chk.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 16, 16)
    chk.envlight((1, 1, 1))
    chk.rect(scenes.AXIS_XY, -10, 10, -10, 10, 0, False, chk.mat_matte(tex=chk.texture_checker((1, 0, 0), (0, 1, 0))), None)
    chk.preprocess()
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.upload(chk.flatten(), chk.flatten_textures())
    assert "texture 0" in str(e.value) and "solid or checker" in str(e.value)
    check("after the refused checker")
    ctx.set_texture_mipmaps(None)
    ctx.upload(chk.flatten(), chk.flatten_textures())
    assert ctx.texture_mipmap_info().n_on == 0


# ---- 6. the schedule's rules for textured scenes -------------------------------------------------------------------------------------------------------------------
def test_whitted_refused_fused_falls_back_and_band_shards_union(ctx):
    be = _scene_mirror(_checker(64, 2), 8.0)
    _upload(ctx, be, [1], bounce_spread=1.0)
    film = np.zeros((H, W, 3), f32)
    p = jp.render_params(W, H, 4, 4, integrator=jp.JP_INTEGRATOR_WHITTED)
    assert jp.hip_lib().jp_render(ctx.h, C.byref(p), film.ctypes.data_as(C.c_void_p)) == -5
    a = _render(ctx, W, H, 4, 4)
    acc = np.zeros_like(a)
    for k in range(2):
        acc += _render(ctx, W, H, 4, 4, band_rows=4, shard_index=k, shard_count=2)
    assert _same(acc, a)
    try:
        ctx.set_options(fused=1)
        _upload(ctx, be, [1], bounce_spread=1.0)
        b = _render(ctx, W, H, 4, 4)
        assert ctx.build_info().fused_last_render == 0 and ctx.texture_mipmap_info().mip_last_render == 1
    finally:
        ctx.set_options()
    assert _same(a, b)
