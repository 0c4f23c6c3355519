"""Camera projections without a GPU (INTEGRATION.md "Projections"): jp_projection_rays -- the function the device runs -- against the float64 restatement of
tests/projection_ref.py, landmarks of the three mappings, the validation of jp_set_projection and of the plan, the host API and the command line's flags."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import projection_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1
W, Hh = 37, 19


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


CORNELL = dict(pos=(278.0, 273.0, 960.0), front=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0, W=W, Hh=Hh)
OBLIQUE = dict(pos=(-3.0, 1.5, 2.0), front=(0.6, -0.3, -0.74), up=(0.1, 1.0, 0.05), vfov=40.0, W=W, Hh=Hh)

KINDS = [("ortho", dict(kind=R.ORTHOGRAPHIC, ortho_scale=0.0)), ("ortho_s", dict(kind=R.ORTHOGRAPHIC, ortho_scale=350.0)), ("equirect", dict(kind=R.EQUIRECT))]
KINDS += [("fisheye_%d_%d" % (fov, fit), dict(kind=R.FISHEYE, fov_deg=float(fov), fit=fit)) for fov in (90, 180, 360) for fit in (R.FIT_DIAGONAL, R.FIT_WIDTH, R.FIT_HEIGHT)]


def _every_pixel(spp, seed):
    """film positions of spp samples of every pixel: the pixel plus a 24-bit fraction, as the counter stream gives them"""
    rng = np.random.default_rng(seed)
    yy, xx, _ = np.meshgrid(np.arange(Hh), np.arange(W), np.arange(spp), indexing="ij")
    n = xx.size
    return np.stack([xx.ravel() + rng.integers(0, 1 << 24, n) / 16777216.0, yy.ravel() + rng.integers(0, 1 << 24, n) / 16777216.0], -1).astype(f32)


# ---- H1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_kw", [CORNELL, OBLIQUE], ids=["cornell", "oblique"])
@pytest.mark.parametrize("name,kw", KINDS, ids=[k[0] for k in KINDS])
def test_projection_rays_against_float64(cam_kw, name, kw):
    cam = _camera(**cam_kw)
    fxfy = _every_pixel(2, 11)
    o, d = jp.projection_rays(cam, jp.projection(**kw), fxfy)
    ro, rd = R.rays(cam, fxfy=fxfy, **kw)
    ed = np.abs(d.astype(np.float64) - rd).max()
    el = np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max()
    print("%s: largest direction error %.3e, largest | |dir| - 1 | %.3e" % (name, ed, el))
    # the thirty-odd fp32 roundings of values <= pi on the way to a direction, each <= 1.9e-7, sum to under 6e-6
    assert ed <= 1e-5
    assert el <= 4e-7
    if kw["kind"] == R.ORTHOGRAPHIC:
        s = R.ortho_scale_of(kw["ortho_scale"])
        size = np.linalg.norm(list(cam.pos)) + s * (np.linalg.norm(list(cam.right)) + np.linalg.norm(list(cam.up)))
        eo = np.abs(o.astype(np.float64) - ro).max()
        print("%s: largest origin error %.3e = %.3e of |pos| + s (|right| + |up|)" % (name, eo, eo / size))
        assert eo <= 1e-5 * size
        lr = np.linalg.norm(list(cam.right))
        assert np.ptp((o.astype(np.float64) - np.array(list(cam.pos))) @ (np.array(list(cam.right)) / lr)) > 0.9 * s * lr      # the origins span the view's width
    else:
        assert np.array_equal(o, np.tile(np.array(list(cam.pos), f32), (len(o), 1)))


def test_perspective_is_the_pinhole_and_has_no_plan():
    cam = _camera(**CORNELL)
    fxfy = _every_pixel(1, 5)
    for p in (None, jp.projection(R.PERSPECTIVE)):
        o, d = jp.projection_rays(cam, p, fxfy)
        lo, ld = jp.lens_rays(cam, None, fxfy)
        assert np.array_equal(o, lo) and np.array_equal(d.view(np.uint32), ld.view(np.uint32))
        assert jp.projection_plan(cam, p) is None
    plan = jp.projection_plan(cam, jp.projection("fisheye", fov_deg=120.0, fit="height"))
    assert C.sizeof(jp.JpProjectionPlan) == 14 * 4 and plan.kind == R.FISHEYE
    assert plan.R == Hh / 2.0 and plan.half_fov == f32(np.radians(60.0)) and plan.gamma0 == R.gamma0(cam, R.FISHEYE, 120.0, R.FIT_HEIGHT)
    assert list(plan.ez) == [0.0, 0.0, -1.0] and list(plan.ex) == [1.0, 0.0, 0.0] and list(plan.ey) == [0.0, 1.0, 0.0]
    assert jp.projection_plan(cam, jp.projection("equirect")).gamma0 == R.gamma0(cam, R.EQUIRECT)
    ortho = jp.projection_plan(cam, jp.projection("ortho"))
    assert ortho.gamma0 == 0.0 and ortho.scale == 1.0


# ---- H2 -------------------------------------------------------------------------------------------------------------------------------------------
def test_landmarks():
    cam = _camera(**CORNELL)                                       # axis-aligned: ex = +x, ey = +y, ez = -z exactly
    ex, ey, ez = np.array([1, 0, 0], f32), np.array([0, 1, 0], f32), np.array([0, 0, -1], f32)
    ulp = 2.0 ** -23
    eq = jp.projection("equirect")
    # 18.5 / 37, 9.5 / 19 and 27.75 / 37 are exact in fp32: a = 0 and a = 0.25, b = 0
    _, d = jp.projection_rays(cam, eq, np.array([[W / 2.0, Hh / 2.0], [0.75 * W, Hh / 2.0], [0.0, Hh / 2.0]], f32))
    assert np.array_equal(d[0], ez)                                # phi = theta = 0: ez * 1 + ex * 0 + ey * 0
    assert np.abs(d[1] - ex).max() <= ulp                          # phi = fp32 pi / 2: the cosine is -4.4e-8
    assert np.abs(d[2] + ez).max() <= ulp                          # column 0: directly behind
    top = np.stack([np.arange(W) + 0.5, np.full(W, 0.5)], -1).astype(f32)       # the top row's pixel centres: theta = pi (1/2 - 1/38), sin = 0.9966
    _, dt = jp.projection_rays(cam, eq, top)
    assert ((dt @ ey) > 0.99).all()
    # fisheye
    fe = jp.projection("fisheye", fov_deg=180.0, fit="width")
    _, d = jp.projection_rays(cam, fe, np.array([[W / 2.0, Hh / 2.0], [0.0, Hh / 2.0]], f32))
    assert np.array_equal(d[0], ez)                                # rho == 0
    theta = np.arctan2(-np.float64(d[1] @ ex), np.float64(d[1] @ ez))
    assert abs(theta - np.pi / 2) <= 1e-6 and abs(d[1] @ ey) == 0.0
    # orthographic: one direction, bit for bit
    for kw in (CORNELL, OBLIQUE):
        c = _camera(**kw)
        _, d = jp.projection_rays(c, jp.projection("ortho", ortho_scale=3.0), _every_pixel(2, 7))
        assert (d.view(np.uint32) == d[0].view(np.uint32)[None]).all()
        f = np.array(list(c.front), np.float64)
        assert np.abs(d[0] - f / np.linalg.norm(f)).max() <= 2 * ulp


# ---- H3 -------------------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(struct_bytes=8), "set JpProjection.struct_bytes to sizeof(JpProjection)"),
    (dict(kind=4), "kind must be"),
    (dict(kind=-1), "kind must be"),
    (dict(ortho_scale=-1.0), "ortho_scale must be finite and > 0"),
    (dict(ortho_scale=float("nan")), "ortho_scale must be finite and > 0"),
    (dict(ortho_scale=float("inf")), "ortho_scale must be finite and > 0"),
    (dict(fov_deg=400.0), "fov_deg must be finite and in (0, 360]"),
    (dict(fov_deg=-10.0), "fov_deg must be finite and in (0, 360]"),
    (dict(fov_deg=float("nan")), "fov_deg must be finite and in (0, 360]"),
    (dict(fit=3), "fit must be"),
    (dict(fit=-1), "fit must be"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS)
def test_validation_refuses(kw, msg):
    p = jp.projection(R.FISHEYE, 2.0, 170.0, R.FIT_WIDTH)
    for k, v in kw.items():
        setattr(p, k, v)
    L = jp.hip_lib()
    assert L.jp_check_projection(C.byref(p)) == INVALID_ARGUMENT
    assert L.jp_last_error().decode().startswith("jp_set_projection: " + msg)
    with pytest.raises(jp.JetPbrtError, match="struct_bytes|kind|ortho_scale|fov_deg|fit"):
        jp.check_projection(p)
    cam = _camera(**CORNELL)
    with pytest.raises(jp.JetPbrtError):                            # the pure host entry points validate the same way
        jp.projection_rays(cam, p, np.zeros((1, 2), f32))
    with pytest.raises(jp.JetPbrtError):
        jp.projection_plan(cam, p)


def test_first_rule_broken_is_reported():
    p = jp.projection(7, -1.0, 999.0, 9)
    with pytest.raises(jp.JetPbrtError, match="kind"):
        jp.check_projection(p)
    p.kind = R.ORTHOGRAPHIC
    with pytest.raises(jp.JetPbrtError, match="ortho_scale"):
        jp.check_projection(p)
    p.ortho_scale = 1.0
    with pytest.raises(jp.JetPbrtError, match="fov_deg"):
        jp.check_projection(p)
    p.fov_deg = 360.0
    with pytest.raises(jp.JetPbrtError, match="fit"):
        jp.check_projection(p)
    p.fit = R.FIT_HEIGHT
    jp.check_projection(p)


def test_validation_accepts_and_the_plan_rule():
    jp.check_projection(None)                                       # NULL: the pinhole
    for kind in (R.PERSPECTIVE, R.ORTHOGRAPHIC, R.EQUIRECT, R.FISHEYE):
        jp.check_projection(jp.projection(kind))                    # zeros: the defaults
        jp.check_projection(jp.projection(kind, 1e-3, 360.0, R.FIT_HEIGHT))
    assert C.sizeof(jp.JpProjection) == 20 and C.sizeof(jp.JpProjectionInfo) == 28
    # rule 6, the plan: a skewed camera carries an orthographic projection, not a panorama or a fisheye
    skew = _camera(**CORNELL)
    skew.up[:] = [0.3 * skew.up[1], skew.up[1], 0.0]
    assert jp.projection_plan(skew, jp.projection("ortho")) is not None
    L = jp.hip_lib()
    n = C.c_int64(0)
    for kind in ("equirect", "fisheye"):
        p = jp.projection(kind)
        assert L.jp_projection_plan(C.byref(skew), C.byref(p), None, 0, C.byref(n)) == INVALID_ARGUMENT and n.value == 0
        assert "perpendicular" in L.jp_last_error().decode()
        with pytest.raises(jp.JetPbrtError, match="perpendicular"):
            jp.projection_rays(skew, p, np.zeros((1, 2), f32))
    barely = _camera(**CORNELL)                                    # |dot| of the unit axes 5e-4: inside the 1e-3 the rule allows
    barely.up[:] = [5e-4 * barely.up[1], barely.up[1], 0.0]
    assert jp.projection_plan(barely, jp.projection("equirect")) is not None
    flat = _camera(**CORNELL)
    flat.front[:] = [0.0, 0.0, 0.0]
    for kind in ("ortho", "equirect", "fisheye"):
        with pytest.raises(jp.JetPbrtError, match="finite positive length"):
            jp.projection_plan(flat, jp.projection(kind))
    nan = _camera(**CORNELL)
    nan.right[0] = float("nan")
    with pytest.raises(jp.JetPbrtError, match="finite positive length"):
        jp.projection_plan(nan, jp.projection("ortho"))
    good = jp.projection_plan(_camera(**CORNELL), jp.projection("equirect"))
    small = C.c_int64(0)
    p = jp.projection("equirect"); cam = _camera(**CORNELL)
    assert L.jp_projection_plan(C.byref(cam), C.byref(p), C.byref(good), 8, C.byref(small)) == INVALID_ARGUMENT and "capacity" in L.jp_last_error().decode()


# ---- H4 -------------------------------------------------------------------------------------------------------------------------------------------
def test_host_api_reaches_the_check():
    be = scenes.HostBackend("projection_host")
    with pytest.raises(RuntimeError, match="no camera"):
        be.set_projection("equirect")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 60.0, 32, 16)
    be.set_projection("ortho", ortho_scale=4.0)
    be.set_projection("equirect")
    be.set_projection("fisheye", fov_deg=220.0, fit="height")
    with pytest.raises(RuntimeError, match=r"jp_set_projection: fov_deg must be finite and in \(0, 360\]"):
        be.set_projection("fisheye", fov_deg=400.0)
    with pytest.raises(RuntimeError, match="jp_set_projection: ortho_scale"):
        be.set_projection("ortho", ortho_scale=-2.0)
    with pytest.raises(RuntimeError, match="jp_set_projection: kind"):
        be.set_projection(9)
    be.set_projection("perspective")


def _cli(*args):
    return subprocess.run([jp.CLI_PATH] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_command_line_flags():
    # no scene id: the flags are parsed and checked, nothing is rendered
    for good in (["--projection", "ortho", "--ortho-scale", "2.5"], ["--projection", "equirect"], ["--projection", "fisheye", "--fisheye-fov", "220", "--fisheye-fit", "height"],
                 ["--projection", "fisheye", "--fisheye-fit", "width"], ["--projection", "perspective"]):
        r = _cli(*good)
        assert r.returncode == 0, (good, r.stderr)
    r = _cli("--projection", "fisheye", "--fisheye-fov", "400")
    assert r.returncode != 0 and "jp_set_projection: fov_deg must be finite and in (0, 360]" in r.stderr
    r = _cli("--projection", "ortho", "--ortho-scale", "-1")
    assert r.returncode != 0 and "jp_set_projection: ortho_scale" in r.stderr
    for bad, word in ((["--projection", "cylindrical"], "--projection must be"), (["--projection", "fisheye", "--fisheye-fit", "circle"], "--fisheye-fit must be"),
                      (["--fisheye-fov", "90"], "need --projection"), (["--projection", "equirect", "--aperture", "2"], "exclude each other")):
        r = _cli(*bad)
        assert r.returncode == 5 and word in r.stderr, (bad, r.stderr)
