"""The thin-lens camera without a GPU (INTEGRATION.md "Lens"): jp_lens_rays -- the function the device runs -- against the float64 restatement of
tests/lens_ref.py, convergence of the lens rays on the plane of focus, the shape and uniformity of the aperture samples, and the validation of
jp_set_lens.  Bounds marked "measured" are four times the largest error this file measured against the float64 restatement; each test prints its figure."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import lens_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1
APERTURES = [(0, 0.0), (3, 0.0), (6, 11.0), (16, -27.5)]           # (blades, rotation_deg)


def _camera(pos, front, up, vfov, W, Hh):
    """FCamera's constructor (camera.h:36-49) in float64, rounded to the fp32 fields of JpCamera"""
    front = np.asarray(front, np.float64); front /= np.linalg.norm(front)
    right = np.cross(front, np.asarray(up, np.float64)); right /= np.linalg.norm(right)
    upv = np.cross(right, front)
    th = np.tan(np.radians(vfov) / 2)
    c = jp.JpCamera()
    c.pos[:] = [float(v) for v in pos]; c.front[:] = [float(v) for v in front]
    c.right[:] = [float(v) for v in right * th * (W / Hh)]; c.up[:] = [float(v) for v in upv * th]
    c.res_x, c.res_y = float(W), float(Hh)
    return c


CORNELL = dict(pos=(278.0, 273.0, 960.0), front=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0, W=48, Hh=32)      # |pos| ~ 1037
OBLIQUE = dict(pos=(-3.0, 1.5, 2.0), front=(0.6, -0.3, -0.74), up=(0.1, 1.0, 0.05), vfov=40.0, W=40, Hh=24)
LENS_OF = {"cornell": (12.5, 700.0), "oblique": (0.05, 4.0)}       # (radius, focus distance) in the camera's scene units


def _draws(rng, n, W, Hh):
    fxfy = np.stack([rng.integers(0, W, n) + rng.integers(0, 1 << 24, n) / 16777216.0, rng.integers(0, Hh, n) + rng.integers(0, 1 << 24, n) / 16777216.0], -1).astype(f32)
    u = (rng.integers(0, 1 << 24, (n, 2)) / 16777216.0).astype(f32)
    return fxfy, u


# ---- H1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam_kw", [("cornell", CORNELL), ("oblique", OBLIQUE)])
@pytest.mark.parametrize("blades,rot", APERTURES)
def test_lens_rays_against_float64(name, cam_kw, blades, rot):
    cam = _camera(**cam_kw)
    radius, focus = LENS_OF[name]
    lens = jp.lens(radius, focus, blades, rot)
    fxfy, u = _draws(np.random.default_rng(100 + blades), 4096, cam_kw["W"], cam_kw["Hh"])
    o, d = jp.lens_rays(cam, lens, fxfy, u)
    ro, rd = R.lens_rays(cam, radius, focus, blades, rot, fxfy, u)
    eo = np.abs(o.astype(np.float64) - ro).max(); ed = np.abs(d.astype(np.float64) - rd).max()
    ulp = R.ulp32(np.linalg.norm(cam_kw["pos"]))
    print("blades %d: largest origin error %.3e (%.2f ulp of |pos|), largest direction error %.3e" % (blades, eo, eo / ulp, ed))
    assert eo <= 2 * ulp
    # measured: 1.47e-07 over the eight cases (the oblique camera, 16 blades; the Cornell camera: 9.8e-08), about 2.5 units of 2^-24 -- the roundings of d0,
    # of d0 * F - off and of the division
    assert ed <= 4 * 1.47e-07
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() <= 2e-7


def test_pinhole_rays_and_the_plan():
    cam = _camera(**CORNELL)
    fxfy, _ = _draws(np.random.default_rng(3), 1024, 48, 32)
    for lens in (None, jp.lens(0.0, 0.0, 0, 0.0)):                  # NULL and radius 0: the pinhole, no plan
        o, d = jp.lens_rays(cam, lens, fxfy)
        ro, rd = R.pinhole_rays(cam, fxfy)
        assert np.array_equal(o, ro.astype(f32)) and np.abs(d - rd).max() <= 2e-7
        assert jp.lens_plan(cam, lens) is None
    p = jp.lens_plan(cam, jp.lens(2.0, 5.0, 6, 11.0))
    ref = R.plan32(cam, 2.0, 5.0, 6, 11.0)
    assert (p.radius, p.focus, p.n_verts) == (2.0, 5.0, 6)
    assert np.array_equal(np.array(p.ex[:], f32), ref["ex"]) and np.array_equal(np.array(p.ey[:], f32), ref["ey"])
    v = np.array([list(r) for r in p.v], f32)
    assert np.array_equal(v[:7], ref["v"]) and np.array_equal(v[6], v[0]) and not v[7:].any()
    assert C.sizeof(jp.JpLensPlan) == 43 * 4
    disk = jp.lens_plan(cam, jp.lens(2.0, 5.0))
    assert disk.n_verts == 0 and not np.array([list(r) for r in disk.v]).any()


# ---- H2 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blades,rot", [(0, 0.0), (5, 20.0)])
@pytest.mark.parametrize("focus", [0.1, 1.0, 31.0, 1000.0, 1e4])
def test_rays_meet_on_the_plane_of_focus(blades, rot, focus):
    cam = _camera(**CORNELL)
    radius = focus / 8                                             # a constant f-number: the geometry of the cone does not change with F
    n = 1000
    _, u = _draws(np.random.default_rng(17), n, 48, 32)
    fxfy = np.tile(np.array([[7.3125, 21.640625]], f32), (n, 1))
    o, d = jp.lens_rays(cam, jp.lens(radius, focus, blades, rot), fxfy, u)
    o = o.astype(np.float64); d = d.astype(np.float64)
    pos, front = R.cam_arrays(cam)[:2]
    fh = front / np.linalg.norm(front)
    target = pos + np.float64(f32(focus)) * R.d0_of(cam, fxfy[:1, 0], fxfy[:1, 1])[0]       # the pinhole's point on the plane of focus
    s = ((target - pos) @ fh - (o - pos) @ fh) / (d @ fh)                                   # reaches the target's depth along front
    err = np.abs(o + d * s[:, None] - target).max()
    unit = R.ulp32(np.linalg.norm(pos)) + 2.0 ** -24 * focus
    print("F = %g, blades %d: the rays miss the pinhole's point by at most %.3e = %.2f x (ulp(|pos|) + 2^-24 F)" % (focus, blades, err, err / unit))
    # measured: at most 0.71 of that unit over the ten cases (F = 1e4, where the direction's rounding travels 1e4 units; 0.12 at F <= 1, the origin's rounding alone)
    assert err <= 4 * 0.71 * unit


def _chi2_quantile_1e6(m):
    """the chi^2 quantile at 1 - 1e-6 for m degrees of freedom: scipy's where it is installed, else Wilson-Hilferty (395.4 against 395.2 at m = 270, 0.05 % high)"""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(1.0 - 1e-6, m))
    except ImportError:
        z = 4.753424                                               # the normal quantile at 1 - 1e-6
        return m * (1.0 - 2.0 / (9.0 * m) + z * np.sqrt(2.0 / (9.0 * m))) ** 3


# ---- H3 -------------------------------------------------------------------------------------------------------------------------------------------
def _unit_points(blades, rot, u):
    """the aperture points jp_lens_rays uses, read back from its origins: a camera at the origin with unit axes and radius 1"""
    cam = jp.JpCamera()
    cam.front[:] = [0.0, 0.0, -1.0]; cam.right[:] = [1.0, 0.0, 0.0]; cam.up[:] = [0.0, 1.0, 0.0]; cam.res_x = cam.res_y = 8.0
    o, _ = jp.lens_rays(cam, jp.lens(1.0, 1.0, blades, rot), np.full((len(u), 2), 4.0, f32), u)
    assert not o[:, 2].any()
    return o[:, 0].astype(np.float64), o[:, 1].astype(np.float64)


@pytest.mark.parametrize("blades,rot", APERTURES)
def test_aperture_shape_and_uniformity(blades, rot):
    n = 1 << 18
    i = np.arange(n)
    key = R.rng_key(77, i & 511, i >> 9, np.zeros(n, np.int64))     # the counter stream, fixed seed: deterministic
    u = np.stack([R.rng_float(key, 2), R.rng_float(key, 3)], -1)
    px, py = _unit_points(blades, rot, u)
    rx, ry = R.unit_sample(u[:, 0], u[:, 1], blades, rot)
    assert np.abs(px - rx).max() <= 4 * 2.0 ** -24 and np.abs(py - ry).max() <= 4 * 2.0 ** -24
    assert np.hypot(px, py).max() <= 1.0 + 2 * 2.0 ** -24           # inside the circumradius
    if blades:
        assert R.inside_polygon(px, py, blades, rot).min() >= -4 * 2.0 ** -24
        area = R.polygon_area(blades)
    else:
        area = np.pi
    # a fixed 32 x 32 grid over [-1, 1]^2; only cells wholly inside the shape count
    G = 32
    edges = np.linspace(-1.0, 1.0, G + 1)
    cx, cy = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    corners = [(edges[cx + a].ravel(), edges[cy + b].ravel()) for a in (0, 1) for b in (0, 1)]
    if blades:
        inside = np.min([R.inside_polygon(x, y, blades, rot) for x, y in corners], 0) > 1e-9
    else:
        inside = np.max([np.hypot(x, y) for x, y in corners], 0) < 1.0 - 1e-9
    counts = np.histogram2d(px, py, bins=[edges, edges])[0].ravel()[inside]
    m = int(inside.sum())
    expect = n * (2.0 / G) ** 2 / area
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    bound = _chi2_quantile_1e6(m)                                  # every cell has its own expectation known a priori: m degrees of freedom
    print("blades %d: %d cells inside, %.1f samples expected per cell, chi^2 = %.1f (bound %.1f)" % (blades, m, expect, chi2, bound))
    assert m >= 100 and chi2 <= bound


@pytest.mark.parametrize("blades,rot", APERTURES[1:])
def test_polygon_edge_draws(blades, rot):
    top = f32(1.0 - 2.0 ** -24)
    u = np.array([[top, 0.0], [top, top], [top, 0.5], [0.0, 0.0], [0.0, top]], f32)
    px, py = _unit_points(blades, rot, u)
    v = R.vertices(blades, rot)
    k, w = R.polygon_selector(u[:, 0], blades)
    assert list(k[:3]) == [blades - 1] * 3 and (w[:3] < 1.0).all() and (w[:3] >= 1.0 - 2.0 ** -20).all()       # u0 -> 1 - 2^-24: k stays n - 1
    # u1 = 0: the point is v[k+1] * sqrt(w), next to the vertex v[n] = v[0]
    assert np.hypot(px[0] - v[0, 0], py[0] - v[0, 1]) <= 2.0 ** -19
    assert np.hypot(px[1] - v[blades - 1, 0], py[1] - v[blades - 1, 1]) <= 2.0 ** -19
    assert R.inside_polygon(px[:3], py[:3], blades, rot).min() >= -4 * 2.0 ** -24
    assert px[3] == 0.0 and py[3] == 0.0 and px[4] == 0.0 and py[4] == 0.0                                     # u0 = 0: w = 0, the centre


def test_debug_sampler_points():
    """JP_SAMPLER_DEBUG draws (0.5, 0.5): the centre of the disk and of a polygon with an even number of blades; a point on the middle blade's axis for an odd one"""
    h = np.array([[0.5, 0.5]], f32)
    for blades in (0, 4, 6, 16):
        px, py = _unit_points(blades, 0.0, h)
        assert px[0] == 0.0 and py[0] == 0.0
    for blades in (3, 5, 7):
        px, py = _unit_points(blades, 0.0, h)
        v = R.vertices(blades, 0.0)
        b = 0.5 * np.sqrt(0.5)
        want = (v[(blades - 1) // 2] + v[(blades + 1) // 2]) * b
        assert np.hypot(px[0] - want[0], py[0] - want[1]) <= 4 * 2.0 ** -24 and np.hypot(px[0], py[0]) > 0.1


# ---- H4 -------------------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(radius=float("nan")), "radius must be finite and >= 0"),
    (dict(radius=float("inf")), "radius must be finite and >= 0"),
    (dict(radius=-0.5), "radius must be finite and >= 0"),
    (dict(focus_distance=0.0), "focus_distance must be finite and > 0 when radius > 0"),
    (dict(focus_distance=-2.0), "focus_distance must be finite and > 0 when radius > 0"),
    (dict(focus_distance=float("inf")), "focus_distance must be finite and > 0 when radius > 0"),
    (dict(focus_distance=float("nan")), "focus_distance must be finite and > 0 when radius > 0"),
    (dict(blades=1), "blades must be 0 (a disk) or 3 .. 16"),
    (dict(blades=2), "blades must be 0 (a disk) or 3 .. 16"),
    (dict(blades=17), "blades must be 0 (a disk) or 3 .. 16"),
    (dict(blades=-3), "blades must be 0 (a disk) or 3 .. 16"),
    (dict(rotation_deg=float("nan")), "rotation_deg must be finite"),
    (dict(rotation_deg=float("-inf")), "rotation_deg must be finite"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS)
def test_validation_refuses(kw, msg):
    args = dict(radius=1.0, focus_distance=5.0, blades=0, rotation_deg=0.0); args.update(kw)
    lens = jp.lens(**args)
    L = jp.hip_lib()
    assert L.jp_check_lens(C.byref(lens)) == INVALID_ARGUMENT
    assert L.jp_last_error().decode() == "jp_set_lens: " + msg
    with pytest.raises(jp.JetPbrtError, match="radius|focus_distance|blades|rotation_deg"):
        jp.check_lens(lens)
    cam = _camera(**CORNELL)
    with pytest.raises(jp.JetPbrtError):                            # the pure host entry points validate the same way
        jp.lens_rays(cam, lens, np.zeros((1, 2), f32), np.zeros((1, 2), f32))
    with pytest.raises(jp.JetPbrtError):
        jp.lens_plan(cam, lens)


def test_validation_accepts():
    jp.check_lens(None)                                             # NULL: the pinhole
    jp.check_lens(jp.lens(0.0, 0.0, 0, 0.0))                        # radius 0: the pinhole, whatever the focus distance
    jp.check_lens(jp.lens(0.0, float("nan"), 0, 0.0))
    for blades in (0, 3, 16):
        jp.check_lens(jp.lens(0.25, 1e-3, blades, 720.0))
    short = jp.lens(1.0, 1.0); short.struct_bytes = 8
    with pytest.raises(jp.JetPbrtError, match="struct_bytes"):
        jp.check_lens(short)
    assert C.sizeof(jp.JpLens) == 20 and C.sizeof(jp.JpLensInfo) == 24
