"""Texture sampling records without a GPU (INTEGRATION.md "Texture sampling"): jp_texture_lookup -- the function the device runs -- bit for bit against the numpy
float32 restatement of tests/tex_sampling_ref.py over every mode, the identity against the lookup without records, exact properties on dyadic coordinates, every
refusal of the validation, the host scene's flattening and the command line's options."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
import tex_sampling_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1
SIZES = [(1, 1), (1, 7), (5, 3), (8, 8)]                             # (w, h)
SCALES = [0.5, 1.0, 2.0, 3.0, 7.25]
OFFSETS = [0.0, 0.5, -0.3, 100.125]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _image(w, h, seed=7):
    return np.random.default_rng(seed + 100 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _edge_values(w, h):
    """+-0, 1, exact integers, texel boundaries k / size, -1e-10, 1 - 2^-24, +-2^24, +-3e38, +-inf, NaN"""
    v = [0.0, -0.0, 1.0, -1e-10, 1.0 - 2.0 ** -24, 2.0 ** 24, -2.0 ** 24, 3e38, -3e38, np.inf, -np.inf, np.nan]
    v += [float(k) for k in range(-3, 5)]
    for size in sorted({w, h}):
        v += [k / size for k in range(-size, 2 * size + 1)]
    return np.array(v, f32)


def _coords(w, h):
    rng = np.random.default_rng(31 * w + h)
    e = _edge_values(w, h)
    grid = np.stack(np.meshgrid(e, e), -1).reshape(-1, 2)
    return np.concatenate([rng.uniform(-4, 5, (4096, 2)).astype(f32), grid]).astype(f32)


def _pair(wu, wv, flt, scale=(1.0, 1.0), offset=(0.0, 0.0)):
    return jp.tex_sampler(wu, wv, flt, scale, offset), R.Sampler(wu, wv, flt, scale, offset)


@pytest.mark.parametrize("size", SIZES)
def test_lookup_equals_the_restatement_bit_for_bit(size):
    """every wrap_u x wrap_v x filter; every scale and every offset of the lists on either axis (the other axis takes the list's next entry); 4096 random
    coordinates in [-4, 5] and the edge set crossed with itself"""
    w, h = size
    img = _image(w, h); uv = _coords(w, h)
    n = 0
    for wu, wv, flt in itertools.product(range(3), range(3), range(3)):
        for i, su in enumerate(SCALES):
            for j, ou in enumerate(OFFSETS):
                sc = (su, SCALES[(i + 1) % len(SCALES)]); of = (ou, OFFSETS[(j + 1) % len(OFFSETS)])
                s, r = _pair(wu, wv, flt, sc, of)
                got = jp.texture_lookup(s, img, uv); want = R.lookup(r, img, uv)
                assert np.array_equal(got, want), (size, wu, wv, flt, sc, of, int((got != want).any(1).sum()))
                n += 1
    assert n == 27 * 20


def test_identity_is_the_lookup_without_records():
    for w, h in SIZES + [(37, 23)]:
        img = _image(w, h); uv = _coords(w, h)
        want = R.nearest_clamp(img, uv)
        assert np.array_equal(jp.texture_lookup(None, img, uv), want)
        for flt in (R.DEFAULT, R.NEAREST):
            assert np.array_equal(jp.texture_lookup(jp.tex_sampler(filter=flt), img, uv), want)
    # the general rules reproduce it for every finite coordinate (a NEAREST + CLAMP record with a scale of 1 up to one ulp is not the identity record)
    img = _image(8, 8); uv = _coords(8, 8); fin = np.isfinite(uv).all(1)
    assert np.array_equal(R.lookup(R.Sampler(R.CLAMP, R.CLAMP, R.NEAREST, (1.0, 1.0), (0.0, -0.0)), img, uv[fin]), R.nearest_clamp(img, uv[fin]))


def _nm_inputs(seed, n):
    """the inputs of the normal-map host test: base normals within 30 degrees of the geometric normal, tangents as a parametrisation gives them, uvs a little
    beyond [0, 1], a random 8 x 4 map with blue >= 160"""
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    ng = unit(rng.normal(size=(n, 3)))
    side = unit(np.cross(ng, rng.normal(size=(n, 3))))
    a = np.radians(rng.uniform(0, 30, n))[:, None]
    nb = np.cos(a) * ng + np.sin(a) * side
    t1 = unit(np.cross(nb, rng.normal(size=(n, 3)))); t2 = np.cross(nb, t1)
    al = rng.uniform(0, 2 * np.pi, n); th = np.radians(rng.uniform(30, 150, n)) * rng.choice([-1.0, 1.0], n)

    def tangent(phi):
        return ((np.cos(phi)[:, None] * t1 + np.sin(phi)[:, None] * t2) + rng.uniform(-0.5, 0.5, (n, 1)) * nb) * rng.uniform(0.1, 3.0, (n, 1))
    dpdu = tangent(al); dpdv = tangent(al + th)
    uv = rng.uniform(-0.1, 1.1, (n, 2))
    rgb = rng.integers(0, 256, (4, 8, 3)).astype(np.uint8); rgb[..., 2] = rng.integers(160, 256, (4, 8))
    return nb.astype(f32), ng.astype(f32), dpdu.astype(f32), dpdv.astype(f32), uv.astype(f32), rgb


def test_perturb_normals_sampled_with_no_or_an_identity_record_is_perturb_normals():
    for strength in (0.25, 1.0, 4.0):
        nb, ng, dpdu, dpdv, uv, rgb = _nm_inputs(11, 4096)
        want, won = jp.perturb_normals(nb, ng, dpdu, dpdv, uv, rgb, strength)
        for s in (None, jp.tex_sampler(), jp.tex_sampler(filter=jp.JP_FILTER_BILINEAR)):
            got, on = jp.perturb_normals_sampled(s, nb, ng, dpdu, dpdv, uv, rgb, strength)
            assert _same(got, want) and np.array_equal(on, won)
        assert won.sum() > 2000


def test_perturb_normals_sampled_is_the_map_looked_up_through_the_record():
    """in the frame T = x, B = y, Nb = z the perturbed normal is the looked-up vector normalised: m / sqrtf((mx mx + my my) + mz mz), bit for bit"""
    rng = np.random.default_rng(5)
    n = 2048
    rgb = rng.integers(0, 256, (4, 8, 3)).astype(np.uint8); rgb[..., 2] = rng.integers(200, 256, (4, 8))
    z = np.tile(np.array([0, 0, 1], f32), (n, 1)); du = np.tile(np.array([1, 0, 0], f32), (n, 1)); dv = np.tile(np.array([0, 1, 0], f32), (n, 1))
    uv = rng.uniform(-2, 3, (n, 2)).astype(f32)
    for wu, wv, sc, of in ((R.REPEAT, R.REPEAT, (3.0, 2.0), (0.25, 0.0)), (R.CLAMP, R.REPEAT, (0.5, 7.25), (-0.3, 0.5)), (R.REPEAT, R.CLAMP, (1.0, 1.0), (0.0, 0.0))):
        s, r = _pair(wu, wv, R.DEFAULT, sc, of)
        ns, on = jp.perturb_normals_sampled(s, z, z, du, dv, uv, rgb, 1.0)
        m = R.nmap_lookup(r, rgb, uv)
        n2 = ((m[:, 0] * m[:, 0]).astype(f32) + (m[:, 1] * m[:, 1]).astype(f32)).astype(f32) + (m[:, 2] * m[:, 2]).astype(f32)
        want = (m / np.sqrt(n2.astype(f32))[:, None]).astype(f32)
        k = on == 1
        assert k.sum() > 1900 and _same(ns[k], want[k])
        assert ((m[~k, 0] == 0) & (m[~k, 1] == 0)).all() and _same(ns[~k], z[~k])


# ---- exact properties on dyadic coordinates ------------------------------------------------------------------------------------------------------------
def _dyadic(n, seed, lo=-4, hi=5, bits=6):
    rng = np.random.default_rng(seed)
    return (rng.integers(lo * 2 ** bits, hi * 2 ** bits, (n, 2)) / 2.0 ** bits).astype(f32)


@pytest.mark.parametrize("flt", [jp.JP_FILTER_NEAREST, jp.JP_FILTER_BILINEAR])
def test_repeat_is_periodic_and_mirror_is_even_about_0_and_1(flt):
    img = _image(8, 8); uv = _dyadic(4096, 3)
    rep = jp.tex_sampler(jp.JP_WRAP_REPEAT, filter=flt)
    base = jp.texture_lookup(rep, img, uv)
    for shift in ((1, 0), (0, -3), (2, 5)):
        assert np.array_equal(jp.texture_lookup(rep, img, (uv + np.array(shift, f32)).astype(f32)), base)
    mir = jp.tex_sampler(jp.JP_WRAP_MIRROR, filter=flt)
    base = jp.texture_lookup(mir, img, uv)
    assert np.array_equal(jp.texture_lookup(mir, img, -uv), base)
    assert np.array_equal(jp.texture_lookup(mir, img, (f32(2) - uv).astype(f32)), base)
    assert len(np.unique(base, axis=0)) > 32


def test_bilinear_at_centres_of_a_constant_image_and_at_midpoints():
    w, h = 8, 4
    img = _image(w, h)
    ii, jj = np.meshgrid(np.arange(w), np.arange(h))
    centres = np.stack([(ii.ravel() + 0.5) / w, 1.0 - (jj.ravel() + 0.5) / h], -1).astype(f32)
    for wrap in range(3):
        s = jp.tex_sampler(wrap, filter=jp.JP_FILTER_BILINEAR)
        assert np.array_equal(jp.texture_lookup(s, img, centres), img[jj.ravel(), ii.ravel()])             # a texel centre returns that texel
        const = np.tile(np.array([17, 200, 255], np.uint8), (h, w, 1))
        assert (jp.texture_lookup(s, const, _dyadic(2048, 9)) == const[0, 0]).all()                        # a constant image stays constant
    # halfway between the centres of columns 2 and 3 in row 1: (unsigned)((a + b) / 2 + 0.5) per channel
    s = jp.tex_sampler(jp.JP_WRAP_CLAMP, filter=jp.JP_FILTER_BILINEAR)
    got = jp.texture_lookup(s, img, np.array([[3.0 / w, 1.0 - 1.5 / h]], f32))[0]
    a = img[1, 2].astype(np.float64); b = img[1, 3].astype(np.float64)
    assert np.array_equal(got, np.floor((a + b) / 2 + 0.5).astype(np.uint8))
    # REPEAT at u = 0 mixes the last and the first column half and half; CLAMP and MIRROR stay on the first
    row = np.array([[0.0, 1.0 - 0.5 / h]], f32)
    mix = np.floor((img[0, w - 1].astype(np.float64) + img[0, 0]) / 2 + 0.5).astype(np.uint8)
    assert np.array_equal(jp.texture_lookup(jp.tex_sampler(jp.JP_WRAP_REPEAT, filter=jp.JP_FILTER_BILINEAR), img, row)[0], mix)
    for wrap in (jp.JP_WRAP_CLAMP, jp.JP_WRAP_MIRROR):
        assert np.array_equal(jp.texture_lookup(jp.tex_sampler(wrap, filter=jp.JP_FILTER_BILINEAR), img, row)[0], img[0, 0])
    assert not np.array_equal(mix, img[0, 0])


def test_tiling_selects_the_texel_of_the_tile():
    """REPEAT + NEAREST with scale (2, 2) on a 2 x 2 image: four texel columns and rows across [0, 1]"""
    img = np.array([[[10, 0, 0], [20, 0, 0]], [[30, 0, 0], [40, 0, 0]]], np.uint8)
    s = jp.tex_sampler(jp.JP_WRAP_REPEAT, filter=jp.JP_FILTER_NEAREST, scale=(2, 2))
    u = (np.arange(4) + 0.5) / 4
    uv = np.stack(np.meshgrid(u, u), -1).reshape(-1, 2).astype(f32)
    got = jp.texture_lookup(s, img, uv)[:, 0].reshape(4, 4)              # [v index (bottom up), u index]
    assert np.array_equal(got, np.array([[30, 40, 30, 40], [10, 20, 10, 20], [30, 40, 30, 40], [10, 20, 10, 20]]))


# ---- validation: one test per rule -----------------------------------------------------------------------------------------------------------------------
def _refused(t, word):
    with pytest.raises(jp.JetPbrtError) as e:
        jp.check_texture_sampling(t)
    assert "status %d" % INVALID_ARGUMENT in str(e.value) and word in str(e.value), str(e.value)


def test_check_accepts_and_counts_active_records():
    ident = jp.tex_sampler()
    assert jp.check_texture_sampling(jp.texture_sampling()) == (0, 0)
    assert jp.check_texture_sampling(jp.texture_sampling(tex=[ident, None, jp.tex_sampler(filter=jp.JP_FILTER_NEAREST)], maps=[ident, jp.tex_sampler(filter=jp.JP_FILTER_BILINEAR)])) == (0, 0)
    t = jp.texture_sampling(tex=[ident, jp.tex_sampler(jp.JP_WRAP_REPEAT), jp.tex_sampler(filter=jp.JP_FILTER_BILINEAR), jp.tex_sampler(scale=(1, 2)), jp.tex_sampler(offset=(0.5, 0))],
                            maps=[jp.tex_sampler(jp.JP_WRAP_CLAMP, jp.JP_WRAP_REPEAT), ident, jp.tex_sampler(scale=(3, 2), offset=(0.25, 0))])
    assert jp.check_texture_sampling(t) == (4, 2)
    assert jp.check_texture_sampling(jp.texture_sampling(tex=[], maps=[])) == (0, 0)
    assert C.sizeof(jp.JpTexSampler) == 28 and C.sizeof(jp.JpTextureSampling) == 32 and C.sizeof(jp.JpTexSamplingInfo) == 48


def test_check_refuses_a_short_struct():
    t = jp.texture_sampling(tex=[None]); t.struct_bytes = 8
    _refused(t, "struct_bytes")


def test_check_refuses_unknown_wrap_and_filter_values():
    _refused(jp.texture_sampling(tex=[jp.tex_sampler(3)]), "texture 0: unknown wrap mode")
    _refused(jp.texture_sampling(tex=[None, jp.tex_sampler(0, -1)]), "texture 1: unknown wrap mode")
    _refused(jp.texture_sampling(tex=[jp.tex_sampler(filter=3)]), "unknown filter")
    _refused(jp.texture_sampling(maps=[jp.tex_sampler(filter=-1)]), "normal map 0: unknown filter")


def test_check_refuses_scales_and_offsets():
    for bad in (0.0, -1.0, np.inf, np.nan):
        _refused(jp.texture_sampling(tex=[jp.tex_sampler(scale=(bad, 1))]), "scale must be finite and > 0")
        _refused(jp.texture_sampling(maps=[jp.tex_sampler(scale=(1, bad))]), "scale must be finite and > 0")
    for bad in (np.inf, -np.inf, np.nan):
        _refused(jp.texture_sampling(tex=[jp.tex_sampler(offset=(0, bad))]), "offset not finite")


def test_check_refuses_mirror_and_nearest_on_a_normal_map():
    _refused(jp.texture_sampling(maps=[jp.tex_sampler(jp.JP_WRAP_MIRROR)]), "JP_WRAP_MIRROR on a normal map")
    _refused(jp.texture_sampling(maps=[jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_MIRROR)]), "JP_WRAP_MIRROR on a normal map")
    _refused(jp.texture_sampling(maps=[jp.tex_sampler(filter=jp.JP_FILTER_NEAREST)]), "filtered bilinearly")
    assert jp.check_texture_sampling(jp.texture_sampling(tex=[jp.tex_sampler(jp.JP_WRAP_MIRROR, filter=jp.JP_FILTER_NEAREST)])) == (1, 0)


def test_check_refuses_counts_out_of_range_and_lookup_refuses_bad_arguments():
    t = jp.texture_sampling(tex=[None]); t.n_textures = -1
    _refused(t, "n_textures out of range")
    t = jp.texture_sampling(maps=[None]); t.n_maps = -2
    _refused(t, "n_maps out of range")
    img = _image(2, 2)
    with pytest.raises(jp.JetPbrtError, match="scale must be finite"):
        jp.texture_lookup(jp.tex_sampler(scale=(0, 1)), img, np.zeros((1, 2), f32))
    with pytest.raises(jp.JetPbrtError, match="JP_WRAP_MIRROR"):
        z = np.zeros((1, 3), f32)
        jp.perturb_normals_sampled(jp.tex_sampler(jp.JP_WRAP_MIRROR), z, z, z, z, np.zeros((1, 2), f32), img)


# ---- the host scene and the command line ---------------------------------------------------------------------------------------------------------------
def _host_scene():
    from jet_pbrt_amd import scenes
    be = scenes.HostBackend("tex_sampling_flatten")
    be.camera((0, 0, 4), (0, 0, -1), (0, 1, 0), 30.0, 8, 8)
    be.pointlight((0, 0, 3), (1, 1, 1))
    return scenes, be


def test_host_scene_flattens_its_sampling_records():
    scenes, be = _host_scene()
    img = _image(4, 4)
    rep = jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_MIRROR, jp.JP_FILTER_BILINEAR, (2, 4), (0.5, 0.25))
    ta = be.texture_image(img, sampling=rep); tb = be.texture_image(img); tc = be.texture_checker((1, 0, 0), (0, 1, 0))
    a = be.mat_matte(tex=ta); b = be.mat_matte(tex=tb); c = be.mat_matte(tex=tc)
    be.rect(scenes.AXIS_XY, -1, 1, -1, 1, 0.0, False, a); be.rect(scenes.AXIS_XY, -2, 2, -2, 2, -1.0, False, b); be.rect(scenes.AXIS_XY, -3, 3, -3, 3, -2.0, False, c)
    be.preprocess()
    t = be.flatten_texture_sampling()
    assert t.n_textures == 3 and be.flatten_textures().contents.n_textures == 3 and not t.map and t.n_maps == 0
    r = t.tex[0]
    assert (r.wrap_u, r.wrap_v, r.filter, r.scale_u, r.scale_v, r.offset_u, r.offset_v) == (1, 2, 2, 2.0, 4.0, 0.5, 0.25)
    for k in (1, 2):
        assert (t.tex[k].wrap_u, t.tex[k].wrap_v, t.tex[k].filter, t.tex[k].scale_u, t.tex[k].scale_v, t.tex[k].offset_u, t.tex[k].offset_v) == (0, 0, 0, 1.0, 1.0, 0.0, 0.0)
    assert jp.check_texture_sampling(t) == (1, 0)
    # the scene's default reaches the image without a record of its own, never the checker; the image's own record wins
    be.set_texture_sampling_default(jp.tex_sampler(jp.JP_WRAP_MIRROR, scale=(3, 3)))
    t = be.flatten_texture_sampling()
    assert (t.tex[0].wrap_u, t.tex[1].wrap_u, t.tex[1].scale_u, t.tex[2].wrap_u) == (1, 2, 3.0, 0) and jp.check_texture_sampling(t) == (2, 0)
    be.set_texture_sampling_default(None); be.texture_set_sampling(ta, None)
    assert be.flatten_texture_sampling() is None                     # identity records only: the scene sets no sampling state
    # a normal map's record
    k = be.normal_map(np.full((4, 8, 3), 200, np.uint8), sampling=jp.tex_sampler(jp.JP_WRAP_REPEAT, scale=(3, 2), offset=(0.25, 0)))
    be.mat_set_normal_map(a, k)
    t = be.flatten_texture_sampling()
    assert t.n_maps == 1 and t.n_textures == 3 and (t.map[0].wrap_u, t.map[0].scale_u, t.map[0].scale_v, t.map[0].offset_u) == (1, 3.0, 2.0, 0.25)
    assert jp.check_texture_sampling(t) == (0, 1)
    be.normal_map_set_sampling(k, None)
    assert be.flatten_texture_sampling() is None
    with pytest.raises(RuntimeError):
        be.texture_set_sampling(tc, rep)                             # a checker has no addressing


def test_command_line_parses_the_sampling_options():
    run = lambda *a: subprocess.run([jp.CLI_PATH] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    r = run()
    assert r.returncode == 0 and all(o in r.stderr for o in ("--texture-wrap clamp|repeat|mirror", "--texture-filter nearest|bilinear", "--texture-tile SU SV", "--normal-wrap clamp|repeat", "--normal-tile SU SV"))
    # without a scene id the command line parses its options and leaves
    good = ["--texture-wrap", "mirror", "--texture-filter", "bilinear", "--texture-tile", "4", "2.5", "--normal-wrap", "repeat", "--normal-tile", "8", "8"]
    assert run(*good).returncode == 0
    for bad in (["--texture-wrap", "tile"], ["--texture-filter", "cubic"], ["--texture-tile", "0", "1"], ["--texture-tile", "2", "x"], ["--texture-tile", "2"],
                ["--normal-wrap", "mirror"], ["--normal-tile", "-1", "1"], ["--normal-tile", "inf", "1"], ["--texture-wrap"]):
        r = run(*bad)
        assert r.returncode == 5 and bad[0] in r.stderr.splitlines()[-1], (bad, r.stderr[-200:])
