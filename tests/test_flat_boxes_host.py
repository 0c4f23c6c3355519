"""The box phase of the flat-shape instances (csrc/jp_device.h: flat_boxes_lean) against flat_boxes, as float32 numpy models of both formulations
("The box phase of the flat-shape instances").  No GPU needed.  Both sides get the same reciprocal value; np.fmin / np.fmax drop
a NaN operand as fminf / fmaxf do; every other operation is one IEEE fp32 operation, as under -ffp-contract=off.  What the model can tell apart is the
closest-hit form, which leaves out the clamp of the far distance against tmax = +inf: it must return the masks of the plain form over the Cornell box's
own flat table (the bytes the upload would copy) and over random boxes, for 10^7 random rays and for rays made to hurt -- direction components 0, -0,
denormal, +-tiny, all three of them at once; origins exactly on padded planes (the 0 * inf NaN).  The shadow form keeps the clamp and differs from
flat_boxes only in how the mask is accumulated, which is the GPU tests' business (tests/test_gpu_flat_boxes.py); it is run here for finite tmax and
tmax < tmin so that the model itself is checked against the plain form's expression tree.  The premise of the argument next to the code is asserted
too: of the two plane distances of an axis at most one is NaN."""
import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

F = np.float32
TINY = np.finfo(F).tiny                       # the smallest normal
SLACK = F(1.000002)
CHUNK = 1 << 17


def rcp(d):
    """the reciprocal both formulations share: 0 and denormals give +-inf (v_rcp_f32 takes a denormal for a zero of its sign)"""
    d = np.where(np.abs(d) < TINY, np.copysign(F(0), d), d).astype(F)
    with np.errstate(divide="ignore", over="ignore"):
        return (F(1) / d).astype(F)


def products(boxes, o, inv):
    """the two plane distances per ray, box and axis, (R, B, 3) each: the subtraction and the multiplication both formulations perform"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (boxes[None, :, 0:3] - o[:, None, :]) * inv[:, None, :], (boxes[None, :, 4:7] - o[:, None, :]) * inv[:, None, :]


def plain_pass(t0, t1, tmin, tmax):
    """flat_boxes: (R, B) bool, box i passes for ray r"""
    with np.errstate(invalid="ignore", over="ignore"):
        n, f = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], tmin[:, None]))
        tf = np.fmin(np.fmin(f[..., 0], f[..., 1]), np.fmin(f[..., 2], tmax[:, None]))
        return tn <= tf * SLACK


def lean_pass(t0, t1, tmin, tmax, inf_tmax):
    """flat_boxes_lean<inf_tmax>: the closest-hit form does not look at tmax"""
    with np.errstate(invalid="ignore", over="ignore"):
        n, f = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], tmin[:, None]))
        fxy = np.fmin(f[..., 0], f[..., 1])
        tf = np.fmin(fxy, f[..., 2]) if inf_tmax else np.fmin(fxy, np.fmin(f[..., 2], tmax[:, None]))
        return tn <= tf * SLACK


def compare(boxes, o, d, tmin, tmax):
    """zero mask differences; the closest-hit form where every tmax is +inf, the shadow form always.  Returns (passes, NaN products) seen"""
    passes = nans = 0
    for a in range(0, len(o), CHUNK):
        s = slice(a, a + CHUNK)
        t0, t1 = products(boxes, o[s], rcp(d[s]))
        ref = plain_pass(t0, t1, tmin[s], tmax[s])
        forms = (False, True) if (tmax[s] == np.inf).all() else (False,)
        for inf_tmax in forms:
            diff = lean_pass(t0, t1, tmin[s], tmax[s], inf_tmax) != ref
            assert not diff.any(), "%d masks differ (inf_tmax=%d), first ray %d" % (diff.any(1).sum(), inf_tmax, a + np.argmax(diff.any(1)))
        assert not (np.isnan(t0) & np.isnan(t1)).any()                   # bmin < bmax: the origin lies on at most one plane of an axis
        passes += int(ref.sum()); nans += int(np.isnan(t0).sum() + np.isnan(t1).sum())
    return passes, nans


@pytest.fixture(scope="module")
def cornell_boxes():
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    b = jp.copy_upload_table(be.flatten(), "flat").view(F).reshape(-1, 8).copy()
    be.close()
    assert 2 <= len(b) <= 32 and (b[:, 0:3] < b[:, 4:7]).all()          # padded: bmin < bmax strictly, the premise of the NaN argument
    return b


@pytest.fixture(scope="module")
def random_boxes():
    rng = np.random.default_rng(5)
    lo = rng.uniform(-100, 500, (32, 3)).astype(F)
    ext = np.where(rng.random((32, 3)) < 0.3, 0.0, rng.uniform(0, 300, (32, 3))).astype(F)     # flat boxes among them, then padded like the upload's
    hi = lo + ext
    pad = F(1e-6) * np.maximum(np.abs(lo), np.abs(hi)) + F(1e-30)
    b = np.zeros((32, 8), F)
    b[:, 0:3] = np.nextafter(lo - pad, F(-np.inf)); b[:, 4:7] = np.nextafter(hi + pad, F(np.inf))
    assert (b[:, 0:3] < b[:, 4:7]).all()
    return b


def random_rays(rng, n, lo=-50.0, hi=600.0):
    o = rng.uniform(lo, hi, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return o, d, np.full(n, 0.001, F), np.full(n, np.inf, F)


def test_random_rays_cornell_table(cornell_boxes):
    """10^7 rays from inside the box, closest-hit and shadow form"""
    n = 10_000_000
    o, d, tmin, tmax = random_rays(np.random.default_rng(1), n, 1.0, 548.0)
    o[:, 2] = -o[:, 2]                                                  # the box spans z in [-559.2, 0]
    passes, _ = compare(cornell_boxes, o, d, tmin, tmax)
    assert n <= passes < n * len(cornell_boxes)                         # every ray ends on a wall, so it enters some leaf; no ray enters all of them


def test_random_rays_random_boxes(random_boxes):
    n = 1 << 20
    o, d, tmin, tmax = random_rays(np.random.default_rng(2), n)
    compare(random_boxes, o, d, tmin, tmax)
    compare(random_boxes, o, d, tmin, np.random.default_rng(3).uniform(0.0, 900.0, n).astype(F))


def test_adversarial_rays(cornell_boxes, random_boxes):
    """direction components 0, -0, denormal, +-tiny and huge-reciprocal normals next to ordinary ones, up to all three at once; origins exactly on padded
    planes, so that 0 * inf NaNs do occur; tmax infinite, finite, below tmin"""
    rng = np.random.default_rng(4)
    n = 1 << 19
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, TINY, -TINY, 2 * TINY, -2 * TINY, 1e-30, -1e-30, 1.0, -1.0], F)
    for boxes in (cornell_boxes, random_boxes):
        o, d, tmin, _ = random_rays(rng, n)
        d = np.where(rng.random((n, 3)) < 0.5, special[rng.integers(0, len(special), (n, 3))], d).astype(F)
        d[: n // 16] = special[rng.integers(0, 6, (n // 16, 3))]                          # no finite reciprocal at all: three infinite ones
        b = rng.integers(0, len(boxes), (n, 3)); side = rng.integers(0, 2, (n, 3)) * 4
        o = np.where(rng.random((n, 3)) < 0.5, boxes[b, side + np.arange(3)[None, :]], o).astype(F)
        _, nans = compare(boxes, o, d, tmin, np.full(n, np.inf, F))
        assert nans > n // 64                                            # the case the argument is about was exercised
        compare(boxes, o, d, tmin, rng.uniform(0.0, 900.0, n).astype(F))
        compare(boxes, o, d, tmin, np.full(n, 0.0005, F))


def test_the_model_bites(cornell_boxes):
    """the comparison is not vacuous: leaving out a clamp that matters (a finite tmax) changes masks"""
    o, d, tmin, _ = random_rays(np.random.default_rng(6), 1 << 14, 1.0, 548.0)
    o[:, 2] = -o[:, 2]
    tmax = np.full(len(o), 100.0, F)
    t0, t1 = products(cornell_boxes, o, rcp(d))
    ref = plain_pass(t0, t1, tmin, tmax)
    assert (lean_pass(t0, t1, tmin, tmax, True) != ref).any() and ref.any() and not ref.all()
