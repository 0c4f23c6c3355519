"""Mip maps without a GPU (INTEGRATION.md "Mip maps"): the host builder, the lookup at a footprint and the cone's step -- the functions the device runs -- bit for
bit against the numpy restatement of tests/mipmap_ref.py, the exact pyramids of two checkers, rho <= 1 as the lookup without mipmaps, and every refusal of the
validation.  The refusals that need an upload are marked gpu."""
import itertools

import numpy as np
import pytest

import jet_pbrt_amd as jp
import mipmap_ref as M
import tex_sampling_ref as TR

f32 = np.float32
INVALID_ARGUMENT = -1
SIZES = [(1, 1), (1, 5), (5, 3), (7, 2), (8, 8), (64, 64)]             # (w, h)


def _image(w, h, seed=11):
    return np.random.default_rng(seed + 100 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _checker(n, cell):
    i = np.arange(n) // cell
    c = (((i[:, None] + i[None, :]) & 1) * 255).astype(np.uint8)
    return np.repeat(c[:, :, None], 3, 2)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("size", SIZES)
def test_chain_equals_the_restatement(size):
    w, h = size
    img = _image(w, h)
    got = jp.build_mip_chain(img); want = M.build_chain(img)
    assert [(l.shape[1], l.shape[0]) for l in got] == M.level_sizes(w, h) == jp.mip_level_sizes(w, h)
    assert len(got) == 1 + int(np.floor(np.log2(max(w, h)))) and got[-1].shape[:2] == (1, 1)
    assert np.array_equal(got[0], img)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_checker_pyramids_are_exact():
    one = jp.build_mip_chain(_checker(64, 1))
    assert len(one) == 7 and all((l == 128).all() for l in one[1:])
    two = jp.build_mip_chain(_checker(64, 2))
    assert np.array_equal(two[1], _checker(32, 1)) and set(np.unique(two[1])) == {0, 255}
    assert all((l == 128).all() for l in two[2:])


def _rhos(n_levels):
    r = [0.0, -1.0, np.nan, np.inf, 1.0, float(np.nextafter(f32(1), f32(2))), 2.0, 3.0, 1e30, 1.5, 2.75, 5.3, float(np.nextafter(f32(2), f32(0)))]
    r += [2.0 ** k for k in range(0, n_levels + 2)]
    return np.array(r, f32)


def _uvs(w, h):
    """texel centres and edges of level 0, negative and beyond 1, and a random set"""
    v = [0.0, 1.0, -0.25, 1.75, -3.0, 4.5, 0.5]
    for size in sorted({w, h}):
        v += [(k + 0.5) / size for k in range(size)][:9] + [k / size for k in range(size + 1)][:9]
    e = np.array(sorted(set(v)), f32)
    grid = np.stack(np.meshgrid(e, e), -1).reshape(-1, 2)
    return np.concatenate([grid, np.random.default_rng(5 * w + h).uniform(-2, 3, (256, 2)).astype(f32)]).astype(f32)


@pytest.mark.parametrize("size", [(5, 3), (8, 8)])
def test_lookup_equals_the_restatement_bit_for_bit(size):
    """every wrap pair x both filters (and no record); every rho of the list against every uv of the list"""
    w, h = size
    img = _image(w, h); uv0 = _uvs(w, h); rh0 = _rhos(len(M.level_sizes(w, h)))
    uv = np.repeat(uv0, len(rh0), 0); rho = np.tile(rh0, len(uv0))
    low = ~(rho > 1)
    cases = [(None, None)]
    for wu, wv, flt in itertools.product(range(3), range(3), (jp.JP_FILTER_NEAREST, jp.JP_FILTER_BILINEAR)):
        sc = (1.0, 1.0) if (wu, wv) == (0, 0) else (2.0, 3.0); of = (0.0, 0.0) if wu == 0 else (0.25, -0.5)
        cases.append((jp.tex_sampler(wu, wv, flt, sc, of), TR.Sampler(wu, wv, flt, sc, of)))
    for s, r in cases:
        got = jp.texture_lookup_mip(s, img, uv, rho); want = M.lookup(r, img, uv, rho)
        assert np.array_equal(got, want), (size, None if r is None else (r.wrap_u, r.wrap_v, r.filter), int((got != want).any(1).sum()))
        assert np.array_equal(got[low], jp.texture_lookup(s, img, uv[low]))          # rho <= 1 (0, -1, NaN, 1): the lookup without mipmaps, byte for byte
    assert low.sum() >= 4 * len(uv0)
    inf = np.isinf(rho)
    assert np.array_equal(jp.texture_lookup_mip(None, img, uv[inf], rho[inf]), jp.texture_lookup(None, img, uv[inf]))   # rho not finite: level 0


def test_lookup_past_the_top_level_is_the_last_texel():
    img = _image(8, 8); top = jp.build_mip_chain(img)[-1][0, 0]
    uv = _uvs(8, 8)
    for r in (8.0, 16.0, 1e30):
        assert (jp.texture_lookup_mip(None, img, uv, np.full(len(uv), r, f32)) == top).all()
    c = jp.texture_lookup_mip(None, _checker(64, 1), uv, np.full(len(uv), 2.0, f32))
    assert (c == 128).all()                                             # every level >= 1 of the 1-texel checker is 128: rho >= 2 reads nothing else


def test_cone_step_equals_the_restatement():
    rng = np.random.default_rng(9)
    n = 4096
    bounce = rng.integers(0, 6, n); spec = rng.integers(0, 2, n); dim = rng.integers(0, 40, n)
    flags = (bounce | (spec << 8) | (dim << 16)).astype(np.int32)
    t = rng.uniform(0.01, 900, n).astype(f32)
    st = np.stack([rng.uniform(0, 5, n), rng.uniform(0, 0.3, n)], -1).astype(f32)
    g0, bs = f32(0.0026), f32(0.125)
    got = jp.mip_cone_step(g0, bs, flags, t, st); want = M.cone_step(g0, bs, flags, t, st)
    assert _same(got, want)
    first = bounce == 0
    junk = st.copy(); junk[:, 0] = np.nan; junk[:, 1] = 1e30
    assert _same(jp.mip_cone_step(g0, bs, flags, t, junk)[first], got[first])         # bounce 0 ignores the incoming state
    assert (got[first, 1] == g0).all() and _same(got[first, 0], (g0 * t[first]).astype(f32))
    sp = ~first & (spec == 1)
    assert _same(got[sp, 1], st[sp, 1])                                 # a specular bounce keeps the spread
    df = ~first & (spec == 0)
    assert (got[df, 1] == np.maximum(st[df, 1], bs)).all() and (got[df, 1] >= st[df, 1]).all() and (st[df, 1] > bs).any() and (st[df, 1] < bs).any()


def test_specular_chain_keeps_the_spread_and_adds_the_width():
    g0, bs = f32(0.004), f32(0.2)
    st = jp.mip_cone_step(g0, bs, [0], [10.0], [[7, 7]])
    for b in (1, 2, 3):
        st = jp.mip_cone_step(g0, bs, [b | 0x100], [5.0], st)
    assert st[0, 1] == g0 and _same(st, M.cone_step(g0, bs, [3 | 0x100], [5.0], M.cone_step(g0, bs, [2 | 0x100], [5.0], M.cone_step(g0, bs, [1 | 0x100], [5.0], M.cone_step(g0, bs, [0], [10.0], [[0, 0]])))))
    st2 = jp.mip_cone_step(g0, bs, [4], [5.0], st)
    assert st2[0, 1] == bs and st2[0, 0] == f32(st[0, 0] + f32(bs * f32(5.0)))
    assert jp.mip_cone_step(g0, bs, [5 | 0x100], [1.0], st2)[0, 1] == bs              # ... and a later specular bounce never lowers it


def test_footprint_equals_the_restatement():
    rng = np.random.default_rng(2)
    width = np.concatenate([rng.uniform(0, 3, 500), [0, np.nan, np.inf, 1, 1]]).astype(f32)
    area = np.concatenate([rng.uniform(0.001, 5e4, 500), [1, 1, 1, 0, np.nan]]).astype(f32)
    for w, h, sc, fs in ((64, 64, (1, 1), 1.0), (5, 3, (2, 3), 0.5), (8, 8, (64, 64), 2.0)):
        got = jp.mip_footprint(width, area, w, h, sc, fs)
        assert _same(got, M.rho(width, area, w, h, sc, fs))
        assert (got[-4:] == 0).all()                                    # rho not finite, A not > 0, A not finite: 0


def test_refusals_and_their_messages():
    ok = jp.texture_mipmaps([0, 1, 1, 0], 2.0, 0.1)
    assert jp.check_texture_mipmaps(ok) == 2 and jp.check_texture_mipmaps(jp.texture_mipmaps([])) == 0

    def refused(m, *words):
        with pytest.raises(jp.JetPbrtError) as e:
            jp.check_texture_mipmaps(m)
        assert "status %d" % INVALID_ARGUMENT in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    m = jp.texture_mipmaps([0, 1]); m.struct_bytes = 0
    refused(m, "struct_bytes")
    refused(jp.texture_mipmaps([0, 1, 2]), "texture 2", "unknown mode")
    refused(jp.texture_mipmaps([0, -1]), "texture 1", "unknown mode")
    for bad in (-1.0, np.nan, np.inf):
        refused(jp.texture_mipmaps([1], footprint_scale=bad), "footprint_scale")
        refused(jp.texture_mipmaps([1], bounce_spread=bad), "bounce_spread")


# ---- the host scene and the command line ---------------------------------------------------------------------------------------------------------------
def test_host_scene_flattens_its_mipmap_modes():
    from jet_pbrt_amd import scenes
    be = scenes.HostBackend("mipmap_flatten")
    be.camera((0, 0, 4), (0, 0, -1), (0, 1, 0), 30.0, 8, 8)
    be.pointlight((0, 0, 3), (1, 1, 1))
    img = _image(4, 4)
    ta = be.texture_image(img); tb = be.texture_image(img); tc = be.texture_checker((1, 0, 0), (0, 1, 0))
    a = be.mat_matte(tex=ta); b = be.mat_matte(tex=tb); c = be.mat_matte(tex=tc)
    be.rect(scenes.AXIS_XY, -1, 1, -1, 1, 0.0, False, a); be.rect(scenes.AXIS_XY, -2, 2, -2, 2, -1.0, False, b); be.rect(scenes.AXIS_XY, -3, 3, -3, 3, -2.0, False, c)
    be.preprocess()
    assert be.flatten_texture_mipmaps() is None                         # every mode OFF: the scene sets no mipmap state
    be.texture_set_mipmaps(ta, True)
    m = be.flatten_texture_mipmaps()
    assert m.n_textures == 3 and [m.mode[k] for k in range(3)] == [1, 0, 0] and (m.footprint_scale, m.bounce_spread) == (0.0, 0.0)
    assert jp.check_texture_mipmaps(m) == 1
    # the scene's default reaches the image without a choice of its own, never the checker; an image's own choice wins
    be.set_texture_mipmap_default(True, 2.0, 0.25); be.texture_set_mipmaps(ta, False)
    m = be.flatten_texture_mipmaps()
    assert [m.mode[k] for k in range(3)] == [0, 1, 0] and (m.footprint_scale, m.bounce_spread) == (2.0, 0.25)
    be.texture_set_mipmaps(ta, None)
    assert [be.flatten_texture_mipmaps().mode[k] for k in range(3)] == [1, 1, 0]
    be.set_texture_mipmap_default(False)
    assert be.flatten_texture_mipmaps() is None
    with pytest.raises(RuntimeError):
        be.texture_set_mipmaps(tc, True)                                # a checker has no pyramid


def test_command_line_parses_the_mipmap_options():
    import subprocess
    run = lambda *a: subprocess.run([jp.CLI_PATH] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    r = run()
    assert r.returncode == 0 and "--texture-mip [--mip-footprint S] [--mip-bounce-spread RAD]" in r.stderr
    # without a scene id the command line parses its options and leaves
    assert run("--texture-mip", "--mip-footprint", "2", "--mip-bounce-spread", "0.25").returncode == 0
    for bad in (["--mip-footprint", "0"], ["--mip-footprint", "x"], ["--mip-footprint", "inf"], ["--mip-bounce-spread", "-1"], ["--mip-bounce-spread", "nan"],
                ["--mip-footprint"], ["--mip-bounce-spread"]):
        r = run("--texture-mip", *bad)
        assert r.returncode == 5 and bad[0] in r.stderr.splitlines()[-1], (bad, r.stderr[-200:])
