"""Procedural textures on the MI355X (INTEGRATION.md "Procedural textures"): jp_procedural_probe -- the lookup k_texel_p runs -- bit for bit against
jp_procedural_lookup on the hostile points and boundary widths of the CPU test, the no-op rule, films that are bit-identical to a SOLID texture's and to the plain
CHECKER's by construction (through k_shade_tex and its MIS / environment / smooth twins), the albedo guide against the host lookup at each pixel's own hit, the ray
cone shared with a mip-mapped image, lanes and the shading order, and the refusals at the upload."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import mipmap_ref as M
import procedural_cases as PC
import procedural_ref as R
import test_oracle_features_host as T

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTERS = ("samples", "closest_rays", "closest_hits", "shadow_rays", "shadow_occluded")
IMG = np.random.default_rng(23).integers(0, 256, (64, 64, 3), dtype=np.uint8)
W, H = 48, 32


@pytest.fixture()
def ctx():
    """a context of its own per test: the records, the mipmap modes and the sampling records are context state"""
    c = jp.Context(0)
    yield c
    c.close()


def _same(a, b):
    return PC.same(a, b)


def _counts(ctx):
    c = ctx.counters()
    return tuple(getattr(c, k) for k in COUNTERS)


def _upload(ctx, be, recs=None, mip=None, textures=None, **kw):
    """the scene's sampling records, its mipmap modes and procedural records (None: no state; a list else), then the textured upload"""
    ctx.set_texture_sampling(be.flatten_texture_sampling())
    ctx.set_texture_mipmaps(None if mip is None else jp.texture_mipmaps(mip, **kw))
    ctx.set_texture_procedurals(None if recs is None else jp.texture_procedurals(recs))
    ctx.upload(be.flatten(), be.flatten_textures() if textures is None else textures)


def _render(ctx, spp=16, depth=6, w=W, h=H, **kw):
    return ctx.render(jp.render_params(w, h, spp, depth, 1234, **kw))


def _walls(res=(W, H), image=True, sphere=True):
    """two walls side by side in the plane z = 0, 12 units from the camera: texture 0 (a checker) on the right one, texture 1 (an image, tiled) on the left one.  A
    path that leaves the plane never meets it again: the two textures never see each other.  A glossy sphere in front adds later bounces and shadow rays."""
    be = scenes.HostBackend("procedural_walls")
    be.camera((0, 0, 12), (0, 0, -1), (0, 1, 0), 50.0, res[0], res[1])
    be.envlight((0.6, 0.7, 0.9))
    be.pointlight((0, 3, 6), (30, 28, 25))
    be.rect(scenes.AXIS_XY, 0, 12, -8, 8, 0, False, be.mat_matte(tex=be.texture_checker((0.875, 0.25, 0.125), (0.125, 0.5, 0.75))), None)
    if image:
        rec = jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_REPEAT, jp.JP_FILTER_BILINEAR, (6.0, 8.0))
        be.rect(scenes.AXIS_XY, -12, 0, -8, 8, 0, False, be.mat_matte(tex=be.texture_image(IMG, sampling=rec)), None)
    if sphere:
        be.sphere((0.5, -1.0, 6.0), 1.0, be.mat_plastic((0.4, 0.4, 0.4), (0.3, 0.3, 0.3), 0.2, True), None)
    be.preprocess()
    return be


# ---- 1. the probe ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PC.KINDS)
def test_probe_equals_the_host_lookup_bit_for_bit(ctx, kind):
    """every record of the kind (both spaces, the identity and a general map) on partial waves and on more than one block"""
    lib = jp.hip_lib()
    assert lib.jp_probe_libm_sincosf() != 0, "the device must reproduce this host's sincosf (the plain checker's branch)"
    be = _walls(sphere=False)
    colours = be.flatten_textures().contents.tex_color
    c_odd, c_even = [colours[k] for k in range(3)], [colours[k] for k in range(3, 6)]
    for rec, d in [r for r in PC.records() if r[1]["kind"] == kind]:
        _upload(ctx, be, [rec, None])
        i = ctx.procedural_info()
        assert (i.n_procedural, i.n_antialiased, i.procedural_last_render) == (1, int(d["antialias"] >= 0), 0) and i.table_bytes_device == 80 + 2 * 4
        for n in (1, 63, 64, 65, 257, 4099):
            p, uv, w = PC.grid(n, seed=n)
            got = ctx.procedural_probe(0, p, uv, w)
            want, _ = jp.procedural_lookup(rec, c_even, c_odd, p, uv, w, texture=0)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (d, n, bad[:5], p[bad[:5]], uv[bad[:5]], w[bad[:5]], got[bad[:5]], want[bad[:5]])
    with pytest.raises(jp.JetPbrtError, match="has no procedural record"):
        ctx.procedural_probe(1, np.zeros((1, 3), f32), (0, 0), 0.0)
    with pytest.raises(jp.JetPbrtError, match="out of range"):
        ctx.procedural_probe(2, np.zeros((1, 3), f32), (0, 0), 0.0)


# ---- 2. the no-op rule -------------------------------------------------------------------------------------------------------------------------------------------
def test_no_op_rule(ctx):
    be = _walls()
    before = jp.device_bytes_in_use()
    _upload(ctx, be)
    film0 = _render(ctx); counts0 = _counts(ctx)
    guides0 = ctx.render_guides(jp.render_params(W, H, 16, 6), 2)
    bytes0 = jp.device_bytes_in_use() - before
    assert ctx.procedural_info().procedural_last_render == 0 and film0.std() > 0.01
    junk = jp.procedural(R.NONE, space=7, octaves=99, gain=-3.0, antialias=5)
    for recs in ([None, None], [junk, junk]):
        _upload(ctx, be, recs)
        film1 = _render(ctx)
        i = ctx.procedural_info()
        assert (i.n_procedural, i.n_antialiased, i.procedural_last_render, i.table_bytes_device) == (0, 0, 0, 0)
        assert _same(film0, film1) and _counts(ctx) == counts0 and ctx.texture_mipmap_info().cone_bytes_device == 0
        assert all(_same(a, b) for a, b in zip(guides0, ctx.render_guides(jp.render_params(W, H, 16, 6), 2)))
        assert jp.device_bytes_in_use() - before <= bytes0
    # a record on a texture no material uses: the upload without it
    t = be.flatten_textures().contents
    t.mat_texture[0] = -1                                                  # (the flattened view, until the next preprocess: the checker stays, no material refers to it)
    films = []
    for recs in (None, [jp.procedural(R.FBM), None]):
        _upload(ctx, be, recs)
        films.append(_render(ctx))
        i = ctx.procedural_info()
        assert (i.n_procedural, i.procedural_last_render, i.table_bytes_device) == (0, 0, 0)
    assert _same(films[0], films[1]) and not _same(films[0], film0)


# ---- 3. equal to SOLID, by construction ----------------------------------------------------------------------------------------------------------------------------
def _copy_textures(tp, types=None, colors=None):
    """a JpTextures of its own over the flattened one (which other tests share): tex_type and tex_color replaced where given"""
    s = tp.contents
    t = jp.JpTextures()
    C.memmove(C.byref(t), C.byref(s), C.sizeof(jp.JpTextures))
    ty = np.array([s.tex_type[k] for k in range(s.n_textures)], np.int32)
    co = np.array([s.tex_color[k] for k in range(6 * s.n_textures)], f32)
    if types is not None:
        ty[:] = types
    if colors is not None:
        co[:] = np.asarray(colors, f32).ravel()
    t.tex_type = ty.ctypes.data_as(C.POINTER(C.c_int32)); t.tex_color = co.ctypes.data_as(C.POINTER(C.c_float))
    t._keep = (ty, co, tp)
    return t


def _apply(ctx, st, opts, textures, recs):
    ctx.set_options()
    ctx.set_options(shade_sort=opts.get("shade_sort", 0), lanes=opts.get("lanes", 0))
    ctx.set_environment_map(st["rgb"], "y")
    ctx.set_light_sampling(st["mode"])
    ctx.set_vertex_normals(st["vn"])
    ctx.set_normal_maps(st["nmaps"])
    ctx.set_texture_sampling(st["sampling"])
    ctx.set_texture_procedurals(None if recs is None else jp.texture_procedurals(recs))
    ctx.upload(st["sp"], textures)
    ctx.set_estimator(st["est"])
    ctx.set_lens(None); ctx.set_film(None)


@pytest.mark.parametrize("family", ["all_tex", "mis_env_tex", "smooth_pick_tex"])
def test_equal_colours_give_the_film_of_the_solid_texture(ctx, family):
    """every checker of the zoo (a rectangle, triangles, a mirror sphere, a disk) becomes a checker of two equal colours (1 / 255) * b under a record of a kind of
    its own: r = c + t * (c - c) = c whatever t is, and (1 / 255) * b is the colour k_shade_tex makes of the byte b.  The same film as the SOLID texture of c."""
    st = T.state_of("zoo", T.FAMILIES[family])
    src = st["textures"].contents
    types = np.array([src.tex_type[k] for k in range(src.n_textures)], np.int32)
    checkers = np.nonzero(types == jp.JP_TEXTURE_CHECKER)[0]
    assert len(checkers) == 4
    colors = np.array([src.tex_color[k] for k in range(6 * src.n_textures)], f32).reshape(-1, 6)
    rng = np.random.default_rng(5)
    recs = [None] * src.n_textures
    kinds = [R.FBM, R.MARBLE, R.TURBULENCE, R.CHECKER_AA]
    for j, k in enumerate(checkers):
        c = (f32(1.0) / f32(255.0)) * rng.integers(40, 230, 3).astype(f32)
        colors[k, :3] = c; colors[k, 3:] = c
        recs[k] = jp.procedural(kinds[j], space=R.UV if j == 1 else R.WORLD, m=PC.SCALED if j % 2 else R.IDENTITY, antialias=-1 if j == 2 else 0)
    solid_types = types.copy(); solid_types[checkers] = jp.JP_TEXTURE_SOLID
    films = []
    for ty, rc, ran in ((types, recs, 1), (solid_types, None, 0), (types, None, 0)):
        _apply(ctx, st, dict(shade_sort=1), _copy_textures(st["textures"], ty, colors), rc)
        films.append((ctx.render(st["params"]), _counts(ctx)))
        i = ctx.procedural_info()
        assert (i.procedural_last_render, i.n_procedural, i.n_antialiased) == (ran, 4 * ran, 3 * ran) and ctx.texture_info().textured_last_render == 1
        assert ctx.texture_mipmap_info().cone_bytes_device >= 8 * ran
    (a, ca), (b, cb), (c, cc) = films
    assert _same(a, b) and ca == cb and a.mean() > 0.01
    assert _same(a, c) and ca == cc                                        # (and the plain checker of two equal colours, for what it is worth)
    # the original colours under the same records show the textures: the equality above is the colours' doing
    _apply(ctx, st, dict(shade_sort=1), st["textures"], recs)
    assert not _same(ctx.render(st["params"]), a)


# ---- 4. equal to CHECKER, by construction ----------------------------------------------------------------------------------------------------------------------------
def test_filtered_checker_without_antialiasing_is_the_checker(ctx):
    be = _walls()
    _upload(ctx, be)
    want = _render(ctx); counts = _counts(ctx)
    _upload(ctx, be, [jp.procedural(R.CHECKER_AA, antialias=-1), None])
    got = _render(ctx)
    i = ctx.procedural_info()
    assert (i.n_procedural, i.n_antialiased, i.procedural_last_render) == (1, 0, 1) and ctx.texture_mipmap_info().cone_bytes_device == 0   # no cone: k_texel_p without one
    assert _same(got, want) and _counts(ctx) == counts
    _upload(ctx, be, [jp.procedural(R.CHECKER_AA), None])                  # antialiased: the far wall's cells blur
    assert not _same(_render(ctx), want) and ctx.texture_mipmap_info().cone_bytes_device >= 8 * W * H


def _colour_of(word, c_even, c_odd):
    """the colour k_shade_tex makes of a side word of texture 0: (1 / 255) * byte under the image tag, the checker's odd (index 0) or even (index 1) colour else"""
    rgb = np.stack([(f32(1.0) / f32(255.0)) * ((word >> (8 * k)) & 0xff).astype(f32) for k in range(3)], -1).astype(f32)
    table = np.array([c_odd, c_even], f32)[(word & 1).astype(np.int64)]
    return np.where((word & R.TAG_IMAGE)[:, None] != 0, rgb, table).astype(f32)


# ---- 5. the albedo guide ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.FBM, R.CHECKER_AA])
def test_albedo_guide_is_the_host_lookup_at_the_first_hit(ctx, kind):
    """a rectangle facing the camera, the debug sampler (the pixel's centre), one guide sample: the albedo is the colour of the host lookup at the pixel's own hit
    point o + t d with the camera ray's cone gamma0 * t, t from the depth guide of the same call"""
    be = _walls(image=False, sphere=False)
    rec = jp.procedural(kind, m=(0.25, 0, 0, 0.5, 0, 0.25, 0, 0, 0, 0, 0.25, 0.25) if kind == R.FBM else (0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0.157))
    # (the camera ray's width at the wall is about 0.35: octaves 0 and 1 of the fBm whole, octave 2 fading, the rest gone; the checker's box a quarter of its period)
    _upload(ctx, be, [rec])
    albedo, _, depth = ctx.render_guides(jp.render_params(W, H, 1, 1, sampler_mode=jp.JP_SAMPLER_DEBUG), 1)
    cam = be.flatten().contents.camera
    front, right, up, pos = (np.array([getattr(cam, k)[j] for j in range(3)], f32) for k in ("front", "right", "up", "pos"))
    X, Y = np.meshgrid(np.arange(W).astype(f32) + f32(0.5), np.arange(H).astype(f32) + f32(0.5))
    a = ((X.ravel() / f32(cam.res_x)).astype(f32) - f32(0.5)).astype(f32); b = (f32(0.5) - (Y.ravel() / f32(cam.res_y)).astype(f32)).astype(f32)
    d = ((front[None, :] + (right[None, :] * a[:, None]).astype(f32)).astype(f32) + (up[None, :] * b[:, None]).astype(f32)).astype(f32)
    l = np.sqrt((((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)).astype(f32)
    d = (d / l[:, None]).astype(f32)
    t = depth.ravel()
    p = (pos[None, :] + (t[:, None] * d).astype(f32)).astype(f32)
    hit = (t > 0) & (p[:, 0] > 0.01)                                         # the right half of the frame: the wall; the left half: the environment
    assert hit.sum() >= W * H // 2 - H and (~hit).sum() >= W * H // 4
    g0 = M.gamma0([cam.up[j] for j in range(3)], cam.res_y)
    colours = be.flatten_textures().contents.tex_color
    c_odd, c_even = [colours[k] for k in range(3)], [colours[k] for k in range(3, 6)]
    word, _ = jp.procedural_lookup(rec, c_even, c_odd, p[hit], (0, 0), (g0 * t[hit]).astype(f32))
    assert (word & R.TAG_IMAGE).all()
    want = _colour_of(word, c_even, c_odd)
    got = albedo.reshape(-1, 3)
    assert _same(got[hit], want) and len(np.unique(word)) > 20
    assert (got[~hit] == 1).all()
    # jp_surface has no cone: width 0
    o = np.tile(pos, (int(hit.sum()), 1))
    _, _, alb = ctx.surface(o, d[hit], np.full(int(hit.sum()), 1e-3, f32), np.full(int(hit.sum()), np.inf, f32))
    word0, _ = jp.procedural_lookup(rec, c_even, c_odd, p[hit], (0, 0), 0.0)
    assert _same(alb, _colour_of(word0, c_even, c_odd)) and bool((word0 & R.TAG_COLOR).all()) == (kind == R.CHECKER_AA)


# ---- 6. the cone is shared with the pyramids -----------------------------------------------------------------------------------------------------------------------------
def test_cone_is_shared_with_a_mip_mapped_image(ctx):
    """the image wall (pyramid) beside the procedural wall (antialiased): the image's side of the probe and of the film is what it is without the record, the
    procedural's side what it is without the pyramid.  No sphere here: a path that leaves the walls' plane never meets it again, so neither texture sees the other."""
    be = _walls(sphere=False)
    n = 1024
    rng = np.random.default_rng(9)
    o = np.tile(f32([0, 0, 12]), (n, 1)); tgt = np.stack([rng.uniform(-11, -0.5, n), rng.uniform(-7, 7, n), np.zeros(n)], -1).astype(f32)
    d = (tgt - o).astype(f32); d = (d / np.sqrt((d * d).sum(1, dtype=f32))[:, None]).astype(f32)
    flags = np.array([0, 1 | 0x100, 1], np.int32)[rng.integers(0, 3, n)]
    st = np.stack([10.0 ** rng.uniform(-2.5, 0.5, n), rng.uniform(0, 0.01, n)], -1).astype(f32)
    args = (o, d, np.full(n, 1e-3, f32), np.full(n, np.inf, f32), flags, st)
    rec = jp.procedural(R.FBM, m=(5, 0, 0, 0, 0, 5, 0, 0, 0, 0, 5, 0))
    _upload(ctx, be, None, [0, 1])
    mip_only = ctx.mip_probe(*args); film_mip = _render(ctx)
    assert ctx.texture_mipmap_info().mip_last_render == 1 and ctx.procedural_info().procedural_last_render == 0
    _upload(ctx, be, [rec, None], None)
    film_proc = _render(ctx)
    assert ctx.texture_mipmap_info().mip_last_render == 0 and ctx.procedural_info().procedural_last_render == 1
    _upload(ctx, be, [rec, None], [0, 1])
    both = ctx.mip_probe(*args); film_both = _render(ctx)
    i = ctx.procedural_info()
    assert (i.n_procedural, i.n_antialiased, i.procedural_last_render) == (1, 1, 1) and ctx.texture_mipmap_info().n_on == 1
    assert (mip_only[1] >= 0).all() and (mip_only[2] > 1).sum() > n // 4 and len(np.unique(mip_only[3], axis=0)) > 50
    assert all(_same(a, b) if a.dtype == f32 else np.array_equal(a, b) for a, b in zip(mip_only, both))
    colours = be.flatten_textures().contents.tex_color
    c_odd, c_even = [colours[k] for k in range(3)], [colours[k] for k in range(3, 6)]
    p, uv, w = PC.grid(257, seed=1)
    assert np.array_equal(ctx.procedural_probe(0, p, uv, w), jp.procedural_lookup(rec, c_even, c_odd, p, uv, w)[0])
    # the films: the camera sits on the seam x = 0, the edge between columns W / 2 - 1 and W / 2 (left out, both); the camera's right axis tells which half shows x < 0
    halves = (slice(0, W // 2 - 1), slice(W // 2 + 1, W))
    image, proc = halves if be.flatten().contents.camera.right[0] > 0 else halves[::-1]
    assert _same(film_both[:, image], film_mip[:, image]) and _same(film_both[:, proc], film_proc[:, proc])
    assert not _same(film_both[:, proc], film_mip[:, proc]) and not _same(film_both[:, image], film_proc[:, image])


# ---- 7. lanes and the shading order ------------------------------------------------------------------------------------------------------------------------------------------
def test_lanes_and_shade_sort_give_the_same_film(ctx):
    be = _walls(res=(64, 64))
    recs = [jp.procedural(R.TURBULENCE, m=(3, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3, 0)), None]
    films = []
    for lanes, sort in ((1, 1), (3, 1), (1, -1), (3, -1)):
        ctx.set_options(lanes=lanes, lane_rows=4, shade_sort=sort)
        _upload(ctx, be, recs, [0, 1])
        films.append(_render(ctx, 8, 6, 64, 64))
        assert ctx.build_info().lanes_last_render == lanes and ctx.procedural_info().procedural_last_render == 1
        assert ctx.texture_mipmap_info().cone_bytes_device >= 8 * 64 * 64
    ctx.set_options()
    assert all(_same(films[0], f) for f in films[1:]) and films[0].std() > 0.01


# ---- 8. refusals at the upload -------------------------------------------------------------------------------------------------------------------------------------------------
def test_upload_refusals_keep_the_scene(ctx, tmp_path):
    be = _walls()
    _upload(ctx, be, [jp.procedural(R.MARBLE), None])
    want = _render(ctx, 2, 2)

    def check(word):
        assert _same(_render(ctx, 2, 2), want), word
        assert ctx.procedural_info().n_procedural == 1, word
    ctx.set_texture_procedurals(jp.texture_procedurals([jp.procedural(R.MARBLE)]))
    with pytest.raises(jp.JetPbrtError) as e:
        ctx.upload(be.flatten(), be.flatten_textures())
    assert "status -1" in str(e.value) and "n_textures (1)" in str(e.value) and "(2)" in str(e.value) and "jp_set_texture_procedurals" in str(e.value)
    check("after a refused textured upload")
    with pytest.raises(jp.JetPbrtError, match="n_textures"):
        ctx.upload(be.flatten())
    check("after a refused plain upload")
    with pytest.raises(jp.JetPbrtError, match="unknown kind"):
        ctx.set_texture_procedurals(jp.texture_procedurals([jp.procedural(9), None]))
    ctx.set_texture_procedurals(jp.texture_procedurals([None, jp.procedural(R.NOISE)]))
    with pytest.raises(jp.JetPbrtError, match="texture 1: a procedural record on a texture that is not JP_TEXTURE_CHECKER"):
        ctx.upload(be.flatten(), be.flatten_textures())
    check("after a record on the image")
    ctx.set_texture_procedurals(jp.texture_procedurals([jp.procedural(R.NOISE), None]))
    hot = _copy_textures(be.flatten_textures(), None, np.array([[1.25, 0, 0, 0, 1, 0], [0] * 6], f32))
    with pytest.raises(jp.JetPbrtError, match=r"texture 0: .*lie in \[0, 1\]"):
        ctx.upload(be.flatten(), hot)
    check("after colours outside [0, 1]")
    # SPACE_UV on triangles without uv
    tri = scenes.HostBackend("procedural_tri")
    tri.camera((0, 0, 12), (0, 0, -1), (0, 1, 0), 50.0, W, H)
    tri.envlight((1, 1, 1))
    obj = scenes.write_obj(str(tmp_path / "tri.obj"), np.array([(-5, -5, 0), (5, -5, 0), (0, 5, 0)], f32), np.array([(0, 1, 2)]))
    tri.mesh(obj, False, False, mat=tri.mat_matte(tex=tri.texture_checker((1, 0, 0), (0, 1, 0))))
    tri.preprocess()
    ctx.set_texture_sampling(None); ctx.set_texture_mipmaps(None)
    bare = _copy_textures(tri.flatten_textures())
    bare.tri_uv = None                                                     # a null tri_uv whatever the flattener emits for a mesh without vt
    assert bare.n_triangles == 1 and not bare.tri_uv
    ctx.set_texture_procedurals(jp.texture_procedurals([jp.procedural(R.FBM, space=R.UV)]))
    with pytest.raises(jp.JetPbrtError, match="tri_uv"):
        ctx.upload(tri.flatten(), bare)
    check("after SPACE_UV without tri_uv")
    ctx.set_texture_procedurals(jp.texture_procedurals([jp.procedural(R.FBM)]))
    ctx.upload(tri.flatten(), tri.flatten_textures())
    assert ctx.procedural_info().n_procedural == 1
    # the Whitted integrator refuses a textured scene as before, the path integrator goes on
    film = np.zeros((H, W, 3), f32)
    pw = jp.render_params(W, H, 2, 2, integrator=jp.JP_INTEGRATOR_WHITTED)
    assert jp.hip_lib().jp_render(ctx.h, C.byref(pw), film.ctypes.data_as(C.c_void_p)) == -5
    assert _render(ctx, 2, 2).std() > 0


# ---- 9. the host API ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_api_hands_the_records_over(ctx):
    """FProceduralTexture through the host library's integrator == the flattened records through the C ABI; a scene without one afterwards removes the state"""
    def scene(procedural):
        be = scenes.HostBackend("procedural_host")
        be.camera((0, 0, 12), (0, 0, -1), (0, 1, 0), 50.0, W, H)
        be.envlight((0.6, 0.7, 0.9))
        odd, even = (0.875, 0.25, 0.125), (0.125, 0.5, 0.75)
        tex = be.texture_procedural(jp.procedural(R.MARBLE, m=(0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0), variation=1.5), odd, even) if procedural else be.texture_checker(odd, even)
        be.rect(scenes.AXIS_XY, -12, 12, -8, 8, 0, False, be.mat_matte(tex=tex), None)
        be.preprocess()
        return be
    films = []
    for procedural in (True, False, True):
        be = scene(procedural)
        film = np.zeros((H, W, 3), f32); cnt = jp.JpCounters()
        assert jp.host_lib().jp_host_render(be.h, W, H, 4, 5, 1234, 0, 0, 1, film.ctypes.data, cnt) == 0
        pr = be.flatten_texture_procedurals()
        assert (pr is not None) == procedural
        ctx.set_texture_procedurals(pr)
        ctx.upload(be.flatten(), be.flatten_textures())
        direct = ctx.render(jp.render_params(W, H, 4, 5, 1234))
        assert ctx.procedural_info().procedural_last_render == int(procedural)
        assert film.mean() > 0.02 and _same(film, direct)
        films.append(film)
    assert _same(films[0], films[2]) and not _same(films[0], films[1])
