"""Normal maps without a GPU (INTEGRATION.md "Normal maps"): jp_perturb_normals -- the function the device runs -- against the float64 restatement of
tests/normal_map_ref.py, its exact cases, the triangle tangents, the directions derived for sphere and disk against finite differences of their uv
functions, and every refusal of jp_set_normal_maps' validation.  Figures these tests print are recorded in DESIGN.md "Normal maps"."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import normal_map_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1
MARGIN = 1e-3                  # a decision of the definition closer to its edge than this may legitimately fall the other way in fp32
# the largest angle between jp_perturb_normals and the float64 restatement measured over the 3 x 4096 points below was 1.765e-6 rad at strength 4 (1.8e-7 at 0.25, 5.1e-7 at 1: fp32 accumulation over
# about 30 operations); 4 x that, the factor covering other inputs, not another implementation
ANGLE_BOUND = 4 * 1.765e-6


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_inputs(seed, n):
    """base normals within 30 degrees of the geometric normal; dpdu and dpdv as a parametrisation gives them: lengths 0.1 .. 3, up to 27 degrees out of
    the tangent plane, 30 .. 150 degrees apart in it on either side (mirrored uvs) -- nearly parallel tangents are ill-conditioned input, not a decision
    edge; uvs a little beyond [0, 1]; a random 8 x 4 map whose z stays positive (blue >= 160) so that most points perturb"""
    rng = np.random.default_rng(seed)
    ng = _unit(rng.normal(size=(n, 3)))
    side = _unit(np.cross(ng, rng.normal(size=(n, 3))))
    a = np.radians(rng.uniform(0, 30, n))[:, None]
    nb = np.cos(a) * ng + np.sin(a) * side
    t1 = _unit(np.cross(nb, rng.normal(size=(n, 3)))); t2 = np.cross(nb, t1)
    al = rng.uniform(0, 2 * np.pi, n); th = np.radians(rng.uniform(30, 150, n)) * rng.choice([-1.0, 1.0], n)

    def tangent(phi):
        return ((np.cos(phi)[:, None] * t1 + np.sin(phi)[:, None] * t2) + rng.uniform(-0.5, 0.5, (n, 1)) * nb) * rng.uniform(0.1, 3.0, (n, 1))
    dpdu = tangent(al); dpdv = tangent(al + th)
    uv = rng.uniform(-0.1, 1.1, (n, 2))
    rgb = rng.integers(0, 256, (4, 8, 3)).astype(np.uint8); rgb[..., 2] = rng.integers(160, 256, (4, 8))
    return nb.astype(f32), ng.astype(f32), dpdu.astype(f32), dpdv.astype(f32), uv.astype(f32), rgb


def test_perturb_normals_is_close_to_float64():
    worst = 0.0
    for strength in (0.25, 1.0, 4.0):
        nb, ng, dpdu, dpdv, uv, rgb = random_inputs(11, 4096)
        got, on = jp.perturb_normals(nb, ng, dpdu, dpdv, uv, rgb, strength)
        ref, ron, margin = R.perturb(nb, ng, dpdu, dpdv, uv, rgb, strength)
        clear = margin > MARGIN
        assert (~clear).mean() <= 0.02                               # at most 2 % of the inputs sit near a decision edge
        assert np.array_equal(on[clear] != 0, ron[clear])
        both = clear & ron & (on != 0)
        ang = R.angle(got[both], ref[both])
        print("strength %.2f: %d points, %d near an edge, %d perturbed by both, largest angle %.3e rad" % (strength, len(on), (~clear).sum(), both.sum(), ang.max()))
        assert both.sum() > 2000
        assert np.abs(np.linalg.norm(got[both].astype(np.float64), axis=-1) - 1.0).max() <= 1e-6
        assert _same(got[on == 0], nb[on == 0])                      # unperturbed: the base normal, bit for bit
        worst = max(worst, ang.max())
    print("largest angle over the three strengths %.3e rad, bound %.3e" % (worst, ANGLE_BOUND))
    assert worst <= ANGLE_BOUND


def _frame_inputs(n=64, seed=3):
    rng = np.random.default_rng(seed)
    z = np.tile(np.array([0.0, 0.0, 1.0], f32), (n, 1))
    dpdu = np.tile(np.array([1.0, 0.0, 0.0], f32), (n, 1)); dpdv = np.tile(np.array([0.0, 1.0, 0.0], f32), (n, 1))
    return z, dpdu, dpdv, rng.uniform(0, 1, (n, 2)).astype(f32)


def test_a_neutral_map_perturbs_nothing_exactly():
    nb, ng, dpdu, dpdv, uv, _ = random_inputs(5, 512)
    rgb = np.zeros((4, 8, 3), np.uint8); rgb[..., 0] = 128; rgb[..., 1] = 128; rgb[..., 2] = 255
    ns, on = jp.perturb_normals(nb, ng, dpdu, dpdv, uv, rgb, 1.0)
    assert (on == 0).all() and _same(ns, nb)
    assert jp.perturb_normals(nb, ng, dpdu, dpdv, uv, rgb, 4.0)[1].sum() == 0


def test_a_one_texel_map_tilts_in_the_t_nb_plane():
    z, dpdu, dpdv, uv = _frame_inputs()
    rgb = np.array([[[200, 128, 230]]], np.uint8)                   # mx = 72 / 127, my = 0 exactly, mz = 102 / 127
    ns, on = jp.perturb_normals(z, z, dpdu, dpdv, uv, rgb, 1.0)
    assert (on == 1).all() and (ns[:, 1] == 0).all()
    want = np.array([72.0, 0.0, 102.0]) / np.hypot(72.0, 102.0)
    assert np.abs(ns.astype(np.float64) - want).max() <= 1e-7
    # a tilted frame: the result stays in the plane of T and Nb
    nb = _unit(np.array([[0.2, -0.1, 1.0]])).astype(f32).repeat(len(z), 0)
    ns, on = jp.perturb_normals(nb, nb, dpdu, dpdv, uv, rgb, 1.0)
    T = dpdu.astype(np.float64) - nb * (nb.astype(np.float64) * dpdu).sum(-1, keepdims=True)
    out_of_plane = np.abs((np.cross(T, nb.astype(np.float64)) * ns).sum(-1))
    assert (on == 1).all() and out_of_plane.max() <= 1e-7


def test_bilinear_lookup_at_centres_midpoints_and_outside():
    rng = np.random.default_rng(9)
    rgb = rng.integers(0, 256, (4, 8, 3)).astype(np.uint8); rgb[..., 2] = rng.integers(200, 256, (4, 8))
    z = np.array([[0.0, 0.0, 1.0]], f32); du = np.array([[1.0, 0.0, 0.0]], f32); dv = np.array([[0.0, 1.0, 0.0]], f32)

    def at(u, v):
        return jp.perturb_normals(z, z, du, dv, np.array([[u, v]], f32), rgb, 1.0)[0][0]

    def texel(i, j):                                                 # the one-texel map of texel (i, j): its own vector
        return jp.perturb_normals(z, z, du, dv, np.array([[0.5, 0.5]], f32), rgb[j:j + 1, i:i + 1], 1.0)[0][0]
    for i, j in ((0, 0), (3, 1), (7, 3), (5, 2)):
        assert _same(at((i + 0.5) / 8.0, 1.0 - (j + 0.5) / 4.0), texel(i, j))      # 8 and 4 are powers of two: the centre is exact in fp32
    # halfway between the centres of texels (2, 1) and (3, 1): the midpoint a + 0.5 (b - a) per component in fp32 (fy is exactly 0), then the definition
    # in this frame, where T, B and Nb are the axes and n is the midpoint itself: n / sqrtf((nx nx + ny ny) + nz nz), bit for bit
    a = R.decode(rgb[1, 2]).astype(f32); b = R.decode(rgb[1, 3]).astype(f32)       # (an integer over 127, correctly rounded: the fp32 quotient)
    mid = (a + f32(0.5) * (b - a)).astype(f32)
    n2 = f32(f32(mid[0] * mid[0]) + f32(mid[1] * mid[1])) + f32(mid[2] * mid[2])
    assert mid.dtype == f32 and _same(at(3.0 / 8.0, 1.0 - 1.5 / 4.0), (mid / np.sqrt(f32(n2))).astype(f32))
    # outside [0, 1]: the edge's texel (clamp addressing), NaN: 0
    assert _same(at(-3.0, 2.0), texel(0, 0)) and _same(at(7.0, -1.0), texel(7, 3)) and _same(at(1.0, 1.0), texel(7, 0))
    assert _same(at(np.nan, np.nan), texel(0, 3))


def test_strength_zero_and_a_normal_below_the_geometric_plane_stay_unperturbed():
    z, dpdu, dpdv, uv = _frame_inputs()
    rgb = np.array([[[250, 128, 140]]], np.uint8)                   # a steep tilt toward +x
    ns, on = jp.perturb_normals(z, z, dpdu, dpdv, uv, rgb, 0.0)
    assert (on == 0).all() and _same(ns, z)
    assert (jp.perturb_normals(z, z, dpdu, dpdv, uv, rgb, 1.0)[1] == 1).all()
    ng = _unit(np.array([[-1.0, 0.0, 0.3]])).astype(f32).repeat(len(z), 0)          # the geometric normal leans the other way: dot(Ns', N) < 0
    ns, on = jp.perturb_normals(z, ng, dpdu, dpdv, uv, rgb, 1.0)
    assert (on == 0).all() and _same(ns, z)
    # a degenerate dpdu (parallel to Nb, or 0) leaves the point alone as well
    assert jp.perturb_normals(z, z, z * f32(2), dpdv, uv, rgb, 1.0)[1].sum() == 0
    assert jp.perturb_normals(z, z, z * f32(0), dpdv, uv, rgb, 1.0)[1].sum() == 0
    # a degenerate dpdv falls back to cross(Nb, T)
    ns, on = jp.perturb_normals(z, z, dpdu, z * f32(0), uv, np.array([[[128, 200, 230]]], np.uint8), 1.0)
    assert (on == 1).all() and (ns[:, 0] == 0).all() and (ns[:, 1] > 0).all()


def test_triangle_tangents_against_float64_and_degenerate_uvs():
    rng = np.random.default_rng(13)
    n = 2048
    p = rng.uniform(-2, 2, (3, n, 3)).astype(f32)
    uv6 = rng.uniform(0, 1, (n, 6)).astype(f32)
    uv6[:8, 2:4] = uv6[:8, 0:2]                                      # uv1 == uv0: det == 0
    uv6[8:16, 4:6] = uv6[8:16, 0:2] + 2 * (uv6[8:16, 2:4] - uv6[8:16, 0:2])     # collinear uvs
    uv6[16, 3] = np.inf
    du, dv, ok = jp.triangle_tangents(p[0], p[1], p[2], uv6)
    rdu, rdv, rok = R.triangle_tangents(p[0], p[1], p[2], uv6)
    det = (uv6[:, 2].astype(np.float64) - uv6[:, 0]) * (uv6[:, 5].astype(np.float64) - uv6[:, 1]) - (uv6[:, 3].astype(np.float64) - uv6[:, 1]) * (uv6[:, 4].astype(np.float64) - uv6[:, 0])
    clear = ~np.isfinite(det) | (np.abs(det) > 1e-3) | (det == 0)
    clear[8:16] = False                                              # collinear up to rounding: either answer
    assert (ok[:8] == 0).all() and ok[16] == 0 and (du[ok == 0] == 0).all() and (dv[ok == 0] == 0).all()
    assert np.array_equal(ok[clear] != 0, rok[clear])
    both = clear & rok
    a = max(R.angle(du[both], rdu[both]).max(), R.angle(dv[both], rdv[both]).max())
    print("triangle tangents: %d triangles, %d compared, largest angle to float64 %.3e rad" % (n, both.sum(), a))
    assert both.sum() > 1500 and a <= 1e-4                           # (cancellation in dv2 e1 - dv1 e2: |det| > 1e-3 keeps it at a few thousand ulp)


def test_mirrored_uvs_give_the_mirrored_bitangent():
    p0 = np.array([[0.0, 0.0, 0.0]], f32); p1 = np.array([[1.0, 0.0, 0.0]], f32); p2 = np.array([[0.0, 1.0, 0.0]], f32)
    plain = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]], f32)
    mirrored = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, -1.0]], f32)     # v runs the other way
    du, dv, ok = jp.triangle_tangents(p0, p1, p2, plain)
    du_m, dv_m, ok_m = jp.triangle_tangents(p0, p1, p2, mirrored)
    assert ok[0] == 1 and ok_m[0] == 1
    assert du[0].tolist() == [1.0, 0.0, 0.0] and dv[0].tolist() == [0.0, 1.0, 0.0]
    assert du_m[0].tolist() == [1.0, 0.0, 0.0] and dv_m[0].tolist() == [0.0, -1.0, 0.0]
    # the same texel then tilts the other way in y
    z = np.array([[0.0, 0.0, 1.0]], f32); rgb = np.array([[[128, 200, 230]]], np.uint8); uv = np.array([[0.5, 0.5]], f32)
    a = jp.perturb_normals(z, z, du, dv, uv, rgb, 1.0)[0][0]; b = jp.perturb_normals(z, z, du_m, dv_m, uv, rgb, 1.0)[0][0]
    assert a[1] > 0.3 and b[1] == -a[1] and a[0] == 0 and b[2] == a[2]


def test_sphere_and_disk_tangents_are_the_gradients_of_their_uv():
    """pins the derived directions: a step along dpdu raises u and leaves v, a step along dpdv raises v and leaves u (central differences in float64)"""
    rng = np.random.default_rng(17)
    d = _unit(rng.normal(size=(512, 3)))
    d = d[(np.abs(d[:, 1]) < 0.95) & (np.hypot(d[:, 0], d[:, 2]) > 0.2) & ~((d[:, 0] < 0) & (np.abs(d[:, 2]) < 0.05))]     # away from the poles and the u seam
    du, dv = R.sphere_tangents(d)
    assert np.abs((du * d).sum(-1)).max() <= 1e-12 and np.abs((dv * d).sum(-1)).max() <= 1e-12
    h = 1e-6
    for step, (gu, gv) in ((du, (1, 0)), (dv, (0, 1))):
        e = _unit(step)
        g = (R.sphere_uv(_unit(d + h * e)) - R.sphere_uv(_unit(d - h * e))) / (2 * h)
        assert (g[:, 0] > 1e-3).all() if gu else np.abs(g[:, 0]).max() <= 1e-6
        assert (g[:, 1] > 1e-3).all() if gv else np.abs(g[:, 1]).max() <= 1e-6
    for normal in ((0.2, -0.3, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
        s, t, n = R.frame(normal)
        r = rng.uniform(0.1, 0.7, 256); phi = rng.uniform(0.1, 2 * np.pi - 0.1, 256)
        v0 = (r * np.cos(phi))[:, None] * s + (r * np.sin(phi))[:, None] * t
        du, dv = R.disk_tangents(normal, v0)
        for step, (gu, gv) in ((du, (1, 0)), (dv, (0, 1))):
            e = _unit(step)
            g = (R.disk_uv(normal, 0.7, v0 + h * e) - R.disk_uv(normal, 0.7, v0 - h * e)) / (2 * h)
            assert (g[:, 0] > 1e-3).all() if gu else np.abs(g[:, 0]).max() <= 1e-6
            assert (g[:, 1] > 1e-3).all() if gv else np.abs(g[:, 1]).max() <= 1e-6


# ---- validation: one test per refusal ------------------------------------------------------------------------------------------------------------------
def _maps(**kw):
    args = dict(maps=[np.full((4, 8, 3), 128, np.uint8)], mat_map=[0, -1], mat_strength=[1.0, 1.0], tri_uv=np.zeros((3, 6), f32))
    args.update(kw)
    return jp.normal_maps(**args)


def _refused(m, word):
    with pytest.raises(jp.JetPbrtError) as e:
        jp.check_normal_maps(m)
    assert "status %d" % INVALID_ARGUMENT in str(e.value) and word in str(e.value), str(e.value)


def test_check_accepts_and_counts_mapped_materials():
    assert jp.check_normal_maps(_maps()) == 1
    assert jp.check_normal_maps(_maps(mat_map=[-1, -1])) == 0
    assert jp.check_normal_maps(_maps(mat_strength=None, tri_uv=None, n_triangles=5)) == 1
    assert jp.check_normal_maps(jp.normal_maps([], [-1, -1])) == 0
    assert C.sizeof(jp.JpNormalMaps) == 88 and C.sizeof(jp.JpNormalMapInfo) == 48


def test_check_refuses_a_short_struct():
    m = _maps(); m.struct_bytes = 8
    _refused(m, "struct_bytes")


def test_check_refuses_a_map_size_out_of_range():
    m = _maps(); m._keep[0][0] = 16385
    _refused(m, "size out of range")
    m = _maps(); m._keep[1][0] = 0
    _refused(m, "size out of range")


def test_check_refuses_an_offset_beyond_the_texels():
    m = _maps(); m._keep[2][0] = 1
    _refused(m, "beyond n_texel_bytes")
    m = _maps(); m._keep[2][0] = -1
    _refused(m, "beyond n_texel_bytes")


def test_check_refuses_more_than_2_31_texels_in_all():
    """nine maps of 16384 x 16384 that share one (never read) texel range: the validation counts the device pool, 9 * 2^28 texels"""
    n = 9
    w = np.full(n, 16384, np.int32); off = np.zeros(n, np.int64); mm = np.array([0], np.int32); one = np.zeros(1, np.uint8)
    m = jp.JpNormalMaps(C.sizeof(jp.JpNormalMaps), n, w.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_int32)),
                        off.ctypes.data_as(C.POINTER(C.c_int64)), 3 << 28, one.ctypes.data_as(C.POINTER(C.c_uint8)), 1, mm.ctypes.data_as(C.POINTER(C.c_int32)), None, 0, None)
    _refused(m, "2^31 texels")
    m.n_maps = 7
    assert jp.check_normal_maps(m) == 1


def test_check_refuses_a_map_index_out_of_range():
    _refused(_maps(mat_map=[1, -1]), "mat_map out of range")
    _refused(_maps(mat_map=[0, -2]), "mat_map out of range")


def test_check_refuses_a_strength_that_is_not_finite():
    _refused(_maps(mat_strength=[1.0, np.inf]), "strength not finite")
    _refused(_maps(mat_strength=[np.nan, 1.0]), "strength not finite")


def test_check_refuses_null_arrays():
    m = _maps(); m.texels = None
    _refused(m, "null map_width")
    m = _maps(); m.mat_map = None
    _refused(m, "null mat_map")


def test_check_refuses_negative_counts():
    m = _maps(); m.n_triangles = -1
    _refused(m, "negative")
    m = _maps(); m.n_maps = -1
    _refused(m, "n_maps out of range")


def test_check_refuses_a_uv_that_is_not_finite():
    uv = np.zeros((3, 6), f32); uv[2, 1] = np.nan
    _refused(_maps(tri_uv=uv), "uv not finite")


# ---- FNormalMap::FromHeight through the host library ----------------------------------------------------------------------------------------------------
def _from_height(grey, scale):
    from jet_pbrt_amd import scenes
    be = scenes.HostBackend("normal_map_from_height")
    return be.normal_map_data(be.normal_map_from_height(grey, scale))


def _encode(c):
    return np.clip(np.floor(127.0 * np.asarray(c, np.float64) + 0.5) + 128.0, 0, 255).astype(np.uint8)


def test_from_height_of_a_plane_is_the_neutral_map():
    for level in (0, 77, 255):
        m = _from_height(np.full((5, 7), level, np.uint8), 3.0)
        assert m.shape == (5, 7, 3) and (m == np.array([128, 128, 255], np.uint8)).all()


def test_from_height_of_a_ramp_is_the_constant_encoded_tilt():
    ramp = np.tile((np.arange(8) * 20).astype(np.uint8), (4, 1))      # dh/dx = 20 / 255 per texel
    m = _from_height(ramp, 2.0)
    n = np.array([-2.0 * 20.0 / 255.0, 0.0, 1.0]); n /= np.linalg.norm(n)
    assert (m[:, 1:-1] == _encode(n)).all() and m[0, 1, 0] < 128 and m[0, 1, 1] == 128
    half = np.array([-2.0 * 10.0 / 255.0, 0.0, 1.0]); half /= np.linalg.norm(half)      # the clamped neighbour halves the difference at the two ends
    assert (m[:, 0] == _encode(half)).all() and (m[:, -1] == _encode(half)).all()
    up = _from_height(np.ascontiguousarray(ramp.T[::-1]), 2.0)        # the same ramp rising toward the top row: tilts in y
    assert (up[1:-1, :] == _encode([0.0, n[0], n[2]])).all()
    # decoded, the ramp's map tilts Ns toward -u
    z = np.array([[0.0, 0.0, 1.0]], f32)
    ns, on = jp.perturb_normals(z, z, np.array([[1.0, 0, 0]], f32), np.array([[0, 1.0, 0]], f32), np.array([[0.5, 0.5]], f32), m, 1.0)
    assert on[0] == 1 and ns[0, 0] < -0.1 and ns[0, 1] == 0


def test_from_height_is_symmetric_under_mirroring():
    rng = np.random.default_rng(23)
    g = rng.integers(0, 256, (6, 9)).astype(np.uint8)
    m = _from_height(g, 1.7)
    mx = _from_height(np.ascontiguousarray(g[:, ::-1]), 1.7)[:, ::-1]
    my = _from_height(np.ascontiguousarray(g[::-1]), 1.7)[::-1]
    assert np.array_equal(mx[..., 0].astype(int), 256 - m[..., 0].astype(int)) and np.array_equal(mx[..., 1:], m[..., 1:])
    assert np.array_equal(my[..., 1].astype(int), 256 - m[..., 1].astype(int)) and np.array_equal(my[..., [0, 2]], m[..., [0, 2]])
    assert (m[..., 2] > 128).all() and (m[..., 0] != 128).any()


def test_host_scene_flattens_its_normal_maps():
    from jet_pbrt_amd import scenes
    be = scenes.HostBackend("normal_map_flatten")
    be.camera((0, 0, 4), (0, 0, -1), (0, 1, 0), 30.0, 8, 8)
    be.pointlight((0, 0, 3), (1, 1, 1))
    a = be.mat_matte((0.5, 0.5, 0.5)); b = be.mat_glass(1.5, (1, 1, 1), (1, 1, 1)); c = be.mat_matte((0.2, 0.2, 0.2))
    be.rect(scenes.AXIS_XY, -1, 1, -1, 1, 0.0, False, a); be.sphere((0, 0, 1), 0.3, b); be.rect(scenes.AXIS_XY, -2, 2, -2, 2, -1.0, False, c)
    be.preprocess()
    assert be.flatten_normal_maps() is None                          # no material carries a map
    k = be.normal_map(R.bump_map(16))
    be.mat_set_normal_map(a, k, 0.5); be.mat_set_normal_map(b, k)    # shared: flattened once; glass may carry one
    m = be.flatten_normal_maps()
    assert m.n_maps == 1 and m.map_width[0] == 16 and m.n_texel_bytes == 16 * 16 * 3 and m.n_materials == 3 and m.n_triangles == 0
    assert [m.mat_map[i] for i in range(3)] == [0, 0, -1] and m.mat_strength[0] == 0.5 and m.mat_strength[1] == 1.0
    assert jp.check_normal_maps(m) == 2
    be.mat_set_normal_map(a, None); be.mat_set_normal_map(b, -1)
    assert be.flatten_normal_maps() is None
    with pytest.raises(RuntimeError):
        be.normal_map(np.zeros((0, 4, 3), np.uint8))
