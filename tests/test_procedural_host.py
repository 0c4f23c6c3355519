"""Procedural textures without a GPU (INTEGRATION.md "Procedural textures"): jp_procedural_lookup -- the function the device runs -- bit for bit against the numpy
restatement of tests/procedural_ref.py on hostile points and on the fade boundaries, the properties of the noise and of the kinds, band-limiting against a
supersampled ground plane, every refusal of the validation, and the no-op rule of the plan."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import procedural_cases as PC
import procedural_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1


@pytest.mark.parametrize("case", range(len(PC.records())))
def test_lookup_equals_the_restatement_bit_for_bit(case):
    rec, d = PC.records()[case]
    p, uv, w = PC.grid()
    word, t = jp.procedural_lookup(rec, PC.C_EVEN, PC.C_ODD, p, uv, w, texture=3)
    rword, rt = R.lookup(d, PC.C_EVEN, PC.C_ODD, p, uv, w, texture=3)
    sure = ~R.fragile(d, p, uv)                                             # (all but the points where the plain checker's parity hangs on a sine's last bit)
    assert sure.mean() > 0.99
    bad = np.nonzero(((word != rword) | (t.view(np.uint32) != rt.view(np.uint32))) & sure)[0]
    assert bad.size == 0, (d, bad[:5], p[bad[:5]], w[bad[:5]], word[bad[:5]], rword[bad[:5]], t[bad[:5]], rt[bad[:5]])


def _noise(q):
    """n(q) through the NOISE kind between the colours 0 and 1: t = 0.5 + 0.5 n"""
    rec, _ = PC.record(R.NOISE)
    return jp.procedural_lookup(rec, (0, 0, 0), (1, 1, 1), q, (0, 0), 0.0)[1]


def test_noise_is_zero_at_lattice_points_and_bounded():
    rng = np.random.default_rng(1)
    lattice = rng.integers(-5000, 5000, (4096, 3)).astype(f32)
    assert (_noise(lattice) == f32(0.5)).all() and (R.noise(lattice[:, 0], lattice[:, 1], lattice[:, 2]) == 0).all()
    q = rng.uniform(-64, 64, (200000, 3)).astype(f32)
    n = R.noise(q[:, 0], q[:, 1], q[:, 2])
    t = _noise(q)
    assert PC.same(t, (f32(0.5) + (f32(0.5) * n).astype(f32)).astype(f32))
    assert np.abs(n).max() <= 1 and np.abs(n).max() > 0.8 and abs(float(n.mean())) < 0.01        # bounded, and not degenerate
    hostile = np.array([(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (2.0 ** 24, 0.5, 0.5), (0.5, 0.5, -2.0 ** 24), (1e30, 0.5, 0.5)], f32)
    assert (_noise(hostile) == f32(0.5)).all()


def test_fbm_with_every_octave_faded_is_the_mid_colour_exactly():
    rec, _ = PC.record(R.FBM, m=PC.SCALED, octaves=7)
    s = R.resolve(dict(kind=R.FBM, m=PC.SCALED))["s"]
    p, uv = PC.points()
    width = f32(np.nextafter(f32(0.5) / s, f32(1)) * f32(1.0001))
    assert f32(width * s) >= f32(0.5)
    word, t = jp.procedural_lookup(rec, PC.C_EVEN, PC.C_ODD, p, uv, width)
    want = R.word_of(PC.C_EVEN, PC.C_ODD, np.array([0.5], f32))[0]
    assert (t == f32(0.5)).all() and (word == want).all()
    sharp, _ = jp.procedural_lookup(rec, PC.C_EVEN, PC.C_ODD, p, uv, 0.0)
    assert (sharp != want).any()


def test_filtered_checker_ends():
    """below the footprint threshold the plain checker's own colour index; at a huge footprint the 50 / 50 blend"""
    rec, _ = PC.record(R.CHECKER_AA)
    rng = np.random.default_rng(2)
    p = rng.uniform(-3, 3, (4096, 3)).astype(f32)
    s = [np.sin((f32(10) * p[:, k]).astype(f32).astype(np.float64)) for k in range(3)]
    safe = np.abs(s[0] * s[1] * s[2]) > 1e-4                                  # (away from the edges, where the last bit of a sine decides)
    odd = (s[0] * s[1] * s[2]) < 0
    for width in (0.0, 1e-4, float(f32(R.CHECKER_MIN / R.TEN_OVER_PI))):
        word, t = jp.procedural_lookup(rec, PC.C_EVEN, PC.C_ODD, p, (0, 0), width, texture=5)
        assert (word[safe] == (R.TAG_COLOR | (2 * 5 + np.where(odd, 0, 1)))[safe]).all() and (t[safe] == odd[safe]).all()
    off, _ = PC.record(R.CHECKER_AA, antialias=-1)
    word, _ = jp.procedural_lookup(off, PC.C_EVEN, PC.C_ODD, p, (0, 0), 1e6, texture=5)
    assert (word & R.TAG_COLOR).all() and not (word & R.TAG_IMAGE).any()
    blend = R.word_of(PC.C_EVEN, PC.C_ODD, np.array([0.5], f32))[0]
    for width in (2000.0, 1e12, np.inf):
        word, t = jp.procedural_lookup(rec, PC.C_EVEN, PC.C_ODD, p, (0, 0), width)
        assert (word == blend).all() and (t == f32(0.5)).all()
    # in between: the odd fraction of a box that covers whole periods tends to a half, and a small box keeps the plain parity
    _, t = jp.procedural_lookup(rec, (0, 0, 0), (1, 1, 1), p, (0, 0), 0.02)
    inside = np.abs(s[0]) * np.abs(s[1]) * np.abs(s[2]) > 0.3
    assert ((t[inside] > 0.5) == odd[inside]).all()
    _, t = jp.procedural_lookup(rec, (0, 0, 0), (1, 1, 1), p, (0, 0), 50.0)
    assert np.abs(t - 0.5).max() < 1e-3


# The ground lies in the middle of a cell of the 3D checker along y (10 y = -pi / 2).  On y = 0, a face of the cells, sin(10 y) is 0 and the plain checker has one
# colour everywhere: there is nothing to alias.
GROUND = -np.pi / 20


def _ground_rows(rec_on, rec_off, rows, W=96, H=64, ss=8):
    """t of the ground plane y = GROUND under a pinhole camera one unit above it: per pixel of the given rows the lookup at the pixel's centre with the cone's width
    gamma0 * t_hit (antialias on), the same with antialias off, and the mean of ss x ss lookups across the pixel at width 0"""
    fov = np.tan(np.radians(30.0))
    gamma0 = 2.0 * fov / H

    def hits(xs, ys):
        X, Y = np.meshgrid(xs, ys)
        d = np.stack([(X / W - 0.5) * 2 * fov * W / H, (0.5 - Y / H) * 2 * fov - 0.05, -np.ones_like(X)], -1).reshape(-1, 3)
        d /= np.linalg.norm(d, axis=1)[:, None]
        t = -1.0 / d[:, 1]
        return (np.array([0.0, 1.0 + GROUND, 0.0]) + t[:, None] * d).astype(f32), t.astype(f32)
    xs = np.arange(W) + 0.5; ys = np.asarray(rows) + 0.5
    p, t = hits(xs, ys)
    on = jp.procedural_lookup(rec_on, (0, 0, 0), (1, 1, 1), p, (0, 0), (f32(gamma0) * t).astype(f32))[1]
    off = jp.procedural_lookup(rec_off, (0, 0, 0), (1, 1, 1), p, (0, 0), (f32(gamma0) * t).astype(f32))[1]
    sub = (np.arange(ss) + 0.5) / ss
    ps, _ = hits((np.arange(W)[:, None] + sub[None, :]).ravel(), (np.asarray(rows)[:, None] + sub[None, :]).ravel())
    fine = jp.procedural_lookup(rec_off, (0, 0, 0), (1, 1, 1), ps, (0, 0), 0.0)[1].astype(np.float64)
    truth = fine.reshape(len(rows), ss, W, ss).mean((1, 3)).ravel()
    return on.astype(np.float64), off.astype(np.float64), truth


@pytest.mark.parametrize("kind", [R.FBM, R.CHECKER_AA])
def test_band_limiting_lowers_the_error_of_far_rows(kind):
    """a comparison, not a threshold: against a 64-sample supersample of each pixel the antialiased lookup has the smaller mean squared error"""
    m = (6, 0, 0, 0, 0, 6, 0, 0, 0, 0, 6, 0) if kind == R.FBM else R.IDENTITY
    rec_on, _ = PC.record(kind, m=m, octaves=8, antialias=1)
    rec_off, _ = PC.record(kind, m=m, octaves=8, antialias=-1)
    on, off, truth = _ground_rows(rec_on, rec_off, rows=range(33, 41))         # the rows just below the horizon (y = 30.4)
    e_on, e_off = float(((on - truth) ** 2).mean()), float(((off - truth) ** 2).mean())
    print("kind %d: mse antialiased %.5f, point-sampled %.5f" % (kind, e_on, e_off))
    assert e_on < e_off


def _textures(types, colors, tri_uv=False, n_triangles=0):
    keep = [(C.c_int32 * len(types))(*types), (C.c_float * (6 * len(types)))(*[float(x) for c in colors for x in c]), (C.c_int32 * 1)(0), (C.c_float * max(1, 6 * n_triangles))()]
    t = jp.JpTextures()
    t.struct_bytes = C.sizeof(jp.JpTextures); t.n_textures = len(types)
    t.tex_type = C.cast(keep[0], C.POINTER(C.c_int32)); t.tex_color = C.cast(keep[1], C.POINTER(C.c_float))
    t.n_materials = 1; t.mat_texture = C.cast(keep[2], C.POINTER(C.c_int32)); t.n_triangles = n_triangles
    if tri_uv:
        t.tri_uv = C.cast(keep[3], C.POINTER(C.c_float))
    t._keep = keep
    return t


GOOD = dict(kind=R.FBM)
BAD_RECORDS = [
    (dict(kind=6), "unknown kind"), (dict(kind=-1), "unknown kind"), (dict(kind=R.FBM, space=2), "unknown space"),
    (dict(kind=R.FBM, m=(np.nan,) + R.IDENTITY[1:]), "m must be finite"), (dict(kind=R.NOISE, m=R.IDENTITY[:11] + (np.inf,)), "m must be finite"),
    (dict(kind=R.MARBLE, m=(1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0)), "singular"), (dict(kind=R.FBM, m=(0,) * 12), "singular"),
    (dict(kind=R.FBM, octaves=13), "octaves"), (dict(kind=R.FBM, octaves=-1), "octaves"),
    (dict(kind=R.FBM, gain=1.5), "gain"), (dict(kind=R.FBM, gain=-0.5), "gain"), (dict(kind=R.FBM, gain=np.nan), "gain"),
    (dict(kind=R.MARBLE, variation=np.inf), "variation"), (dict(kind=R.FBM, antialias=2), "antialias"),
]


@pytest.mark.parametrize("case", range(len(BAD_RECORDS)))
def test_refusals_of_a_record(case):
    d, msg = BAD_RECORDS[case]
    with pytest.raises(jp.JetPbrtError, match=msg) as e:
        jp.check_texture_procedurals(jp.texture_procedurals([None, jp.procedural(**d)]))
    assert "texture 1" in str(e.value) and "status -1" in str(e.value)
    with pytest.raises(jp.JetPbrtError, match=msg):
        jp.procedural_lookup(jp.procedural(**d), (0, 0, 0), (1, 1, 1), np.zeros((1, 3), f32), (0, 0), 0.0)


def test_refusals_of_the_list_and_of_the_textures():
    v = jp.texture_procedurals([jp.procedural(R.FBM)])
    v.struct_bytes -= 1
    with pytest.raises(jp.JetPbrtError, match="struct_bytes"):
        jp.check_texture_procedurals(v)
    checker = [(1, 0, 0, 0, 1, 0)]
    ok = jp.texture_procedurals([jp.procedural(R.FBM)])
    assert jp.check_texture_procedurals(ok, _textures([jp.JP_TEXTURE_CHECKER], checker)) == (1, 1)
    assert jp.check_texture_procedurals(jp.texture_procedurals([jp.procedural(R.FBM, antialias=-1), None]), _textures([jp.JP_TEXTURE_CHECKER, jp.JP_TEXTURE_SOLID], checker * 2)) == (1, 0)
    with pytest.raises(jp.JetPbrtError, match="n_textures"):
        jp.check_texture_procedurals(ok, _textures([jp.JP_TEXTURE_CHECKER] * 2, checker * 2))
    for ty in (jp.JP_TEXTURE_SOLID, jp.JP_TEXTURE_IMAGE):
        with pytest.raises(jp.JetPbrtError, match="not JP_TEXTURE_CHECKER"):
            jp.check_texture_procedurals(ok, _textures([ty], checker))
    for bad in ((1.5, 0, 0, 0, 1, 0), (1, 0, 0, 0, -0.25, 0), (1, 0, 0, 0, 1, np.nan)):
        with pytest.raises(jp.JetPbrtError, match=r"lie in \[0, 1\]"):
            jp.check_texture_procedurals(ok, _textures([jp.JP_TEXTURE_CHECKER], [bad]))
    uv = jp.texture_procedurals([jp.procedural(R.FBM, space=R.UV)])
    with pytest.raises(jp.JetPbrtError, match="tri_uv"):
        jp.check_texture_procedurals(uv, _textures([jp.JP_TEXTURE_CHECKER], checker, tri_uv=False, n_triangles=2))
    assert jp.check_texture_procedurals(uv, _textures([jp.JP_TEXTURE_CHECKER], checker, tri_uv=True, n_triangles=2)) == (1, 1)
    assert jp.check_texture_procedurals(uv, _textures([jp.JP_TEXTURE_CHECKER], checker, tri_uv=False, n_triangles=0)) == (1, 1)     # (no triangle: rectangles, spheres and disks have their own uv)
    # a failed check leaves the library usable
    assert jp.check_texture_procedurals(ok) == (1, 1)


def test_all_none_is_no_record():
    """The no-op rule on the host: a list of NONE records counts no procedural, whatever else the records hold.  That count is all the host can say about the
    plan: jp_describe_upload takes neither a context nor records, so "the same description with all-NONE records" holds trivially and is not tested here.  The
    rule itself -- the same kernels, film bits, counters and device bytes as the upload without the call -- is checked on an upload, in
    tests/test_gpu_procedural.py::test_no_op_rule."""
    junk = jp.procedural(R.NONE, space=7, m=(np.nan,) * 12, octaves=99, gain=-3.0, antialias=5)
    assert jp.check_texture_procedurals(jp.texture_procedurals([None, junk, None])) == (0, 0)
    assert jp.check_texture_procedurals(jp.texture_procedurals([])) == (0, 0)
    empty = jp.JpTextureProcedurals(C.sizeof(jp.JpTextureProcedurals), 4, None)
    assert jp.check_texture_procedurals(empty) == (0, 0)
    with pytest.raises(jp.JetPbrtError, match="JP_PROC_NONE"):
        jp.procedural_lookup(junk, (0, 0, 0), (1, 1, 1), np.zeros((1, 3), f32), (0, 0), 0.0)


def test_struct_layouts_match_the_header():
    assert C.sizeof(jp.JpProcedural) == 72 and jp.JpProcedural.octaves.offset == 56 and jp.JpProcedural.antialias.offset == 68
    assert C.sizeof(jp.JpTextureProcedurals) == 16 and C.sizeof(jp.JpProceduralInfo) == 24


def test_flattening_and_the_baked_normal_map():
    """FProceduralTexture flattens as the CHECKER of its two colours plus its record, once per texture object; FNormalMap::FromProcedural bakes the host lookup"""
    from jet_pbrt_amd import scenes
    be = scenes.HostBackend("procedural_flat")
    be.camera((0, 0, 12), (0, 0, -1), (0, 1, 0), 50.0, 16, 16)
    be.envlight((1, 1, 1))
    rec = jp.procedural(R.MARBLE, m=PC.SCALED, octaves=4, gain=0.75, variation=2.5, antialias=-1)
    plain = be.texture_checker((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    marble = be.texture_procedural(rec, (1.0, 0.0, 0.25), (0.0, 1.0, 0.5))
    be.rect(scenes.AXIS_XY, 0, 4, -4, 4, 0, False, be.mat_matte(tex=plain), None)
    be.rect(scenes.AXIS_XY, -4, 0, -4, 4, 0, False, be.mat_matte(tex=marble), None)
    be.rect(scenes.AXIS_XY, -8, -4, -4, 4, 0, False, be.mat_mirror(tex=marble), None)            # the same texture object: flattened once
    be.preprocess()
    t = be.flatten_textures().contents
    pr = be.flatten_texture_procedurals()
    assert t.n_textures == 2 and [t.tex_type[k] for k in range(2)] == [jp.JP_TEXTURE_CHECKER] * 2
    assert [t.tex_color[6 + k] for k in range(6)] == [1.0, 0.0, 0.25, 0.0, 1.0, 0.5] and [t.mat_texture[k] for k in range(t.n_materials)] == [0, 1, 1]
    assert pr is not None and pr.n_textures == 2 and pr.rec[0].kind == R.NONE
    r = pr.rec[1]
    assert (r.kind, r.space, r.octaves, r.gain, r.variation, r.antialias) == (R.MARBLE, R.WORLD, 4, 0.75, 2.5, -1) and tuple(r.m) == PC.SCALED
    assert jp.check_texture_procedurals(pr, t) == (1, 0)
    with pytest.raises(RuntimeError, match="unknown kind"):
        be.texture_procedural(jp.procedural(9), (1, 1, 1), (0, 0, 0))
    # a scene without one sets no state
    none = scenes.HostBackend("procedural_none")
    none.camera((0, 0, 12), (0, 0, -1), (0, 1, 0), 50.0, 16, 16)
    none.envlight((1, 1, 1))
    none.rect(scenes.AXIS_XY, 0, 4, -4, 4, 0, False, none.mat_matte(tex=none.texture_checker((1, 0, 0), (0, 1, 0))), None)
    none.preprocess()
    assert none.flatten_texture_procedurals() is None
    # the baked map: heights t over uv in [0, 1)^2 at the texels' centres (row 0 on top, v = 1 there), then FromHeight
    w, h = 24, 10
    got = be.normal_map_data(be.normal_map_from_procedural(rec, w, h, 3.0))
    i, j = np.meshgrid(np.arange(w), np.arange(h))
    uv = np.stack([((i.ravel().astype(f32) + f32(0.5)) / f32(w)).astype(f32), (f32(1) - ((j.ravel().astype(f32) + f32(0.5)) / f32(h)).astype(f32)).astype(f32)], -1)
    d = dict(kind=R.MARBLE, space=R.UV, m=PC.SCALED, octaves=4, gain=0.75, variation=2.5, antialias=-1)
    _, tt = R.lookup(d, (0, 0, 0), (1, 1, 1), np.zeros((w * h, 3), f32), uv, 0.0)
    grey = R.byte(tt).astype(np.uint8).reshape(h, w)
    want = be.normal_map_data(be.normal_map_from_height(grey, 3.0))
    assert got.shape == (h, w, 3) and np.array_equal(got, want) and len(np.unique(grey)) > 20
    with pytest.raises(RuntimeError, match="refuses"):
        be.normal_map_from_procedural(jp.procedural(R.FBM, gain=2.0), 8, 8, 1.0)
