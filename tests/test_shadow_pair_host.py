"""Two shadow rays of one entry in one pass (csrc/jp_device.h: flat_boxes_lean_pair / flat_prims_pair; DESIGN.md section 5, "Shadow pairs") against
the walk they replace, as float32 numpy models of both forms.  No GPU needed.

  sequential   per ray: flat_boxes_lean<false> (subtract, multiply by the reciprocal, min / max, clamp, slack compare), then flat_prims<any-hit>: the
               ray's own mask in __ffs order, tri_hit / rect_hit, return at the first accept
  pair         one box sweep with the six (plane - o) computed once per leaf; one loop over the set bits of mA | mB: record, oa and dot(n, oa) once,
               per ray the division and the interval test, the cross products once if either ray passes, per ray the dot products and the sign
               test; a ray counts a candidate only if ITS OWN mask holds the bit, drops its mask when its verdict closes, and the loop ends when
               no open ray has a candidate left

Every operation is one IEEE fp32 operation, as under -ffp-contract=off; np.fmin / np.fmax drop a NaN as fminf / fmaxf do.  Expected: zero differences in
both masks and both verdicts over more than 10^6 origin / two-direction sets: the Cornell box's own tables (the bytes the upload would copy) under lamp
rays, random triangle / rectangle tables of 32 primitives, origins exactly on primitive planes and on padded box planes, direction components 0, -0 and
denormal, tmax equal for both rays and wildly different -- and tables whose leaf boxes were shrunk on purpose, so that a primitive lies in mB only and
WOULD accept for ray A: the own-mask gating is what keeps A's verdict then (test_foreign_bits_are_never_counted prints and asserts how many such cases
there were; a pair loop without the gating gives other verdicts there)."""
import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

F = np.float32
U = np.uint32
TINY = np.finfo(F).tiny
SLACK = F(1.000002)
TMIN = F(0.001)
CHUNK = 1 << 16
TRIANGLE, RECTANGLE = 0, 1                      # JP_SHAPE_* (include/jetpbrt_amd.h)

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


# ---- shared arithmetic ---------------------------------------------------------------------------------------------------------------
def rcp(d):
    """0 and denormals give +-inf (v_rcp_f32 takes a denormal for a zero of its sign)"""
    d = np.where(np.abs(d) < TINY, np.copysign(F(0), d), d).astype(F)
    with np.errstate(all="ignore"):
        return (F(1) / d).astype(F)


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def cross(a, v):
    return np.stack([a[:, 1] * v[:, 2] - a[:, 2] * v[:, 1], a[:, 2] * v[:, 0] - a[:, 0] * v[:, 2], a[:, 0] * v[:, 1] - a[:, 1] * v[:, 0]], 1)


def same_sign(vs):
    neg = np.ones(len(vs[0]), bool); pos = np.ones(len(vs[0]), bool)
    for v in vs:
        neg &= v < 0; pos &= v >= 0
    return neg | pos


def box_pass(t0, t1, tmax):
    """flat_boxes_lean<false>'s expression tree from the two plane distances per axis -> (R, L) bool"""
    n, f = np.fmin(t0, t1), np.fmax(t0, t1)
    tn = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], TMIN))
    fxy = np.fmin(f[..., 0], f[..., 1])
    tf = np.fmin(fxy, np.fmin(f[..., 2], tmax[:, None]))
    return tn <= tf * SLACK


def to_mask(passes, bits):
    return np.bitwise_or.reduce(np.where(passes, bits[None, :], U(0)), axis=1).astype(U)


# ---- the sequential form -------------------------------------------------------------------------------------------------------------
def boxes_single(flat, o, d, tmax):
    inv = rcp(d)
    t0 = (flat[None, :, 0:3] - o[:, None, :]) * inv[:, None, :]
    t1 = (flat[None, :, 4:7] - o[:, None, :]) * inv[:, None, :]
    return to_mask(box_pass(t0, t1, tmax), flat[:, 3].view(U))


def accept_single(rec, o, d, tmax):
    """prim_hit<FeatFlat>: tri_hit / rect_hit on the records rec (K, 16) -> bool"""
    n = rec[:, 12:15]
    oa = rec[:, 0:3] - o
    dist = dot(n, oa) / dot(n, d)
    ok = (dist > TMIN) & (dist < tmax)
    ob = rec[:, 4:7] - o; oc = rec[:, 8:11] - o
    tri = rec[:, 15].view(np.int32) == TRIANGLE
    v0 = cross(oc, ob); v1 = cross(ob, oa)
    v2t = cross(oa, oc)
    od = np.stack([rec[:, 3], rec[:, 7], rec[:, 11]], 1) - o
    v2r = cross(oa, od); v3r = cross(od, oc)
    in_t = same_sign([dot(v0, d), dot(v1, d), dot(v2t, d)])
    in_r = same_sign([dot(v0, d), dot(v1, d), dot(v2r, d), dot(v3r, d)])
    return ok & np.where(tri, in_t, in_r)


def lowest(m):
    """(bit, index) of the lowest set bit of every word (all non-zero)"""
    bit = (m & (~m + U(1))).astype(U)
    return bit, np.log2(bit.astype(np.float64)).astype(np.int64)


def prims_single(mask, prims, o, d, tmax):
    """flat_prims<any-hit>: the ray's own mask in __ffs order, return at the first accept -> verdict"""
    m = mask.copy(); hit = np.zeros(len(m), bool)
    while True:
        idx = np.nonzero(m)[0]
        if not len(idx):
            return hit
        bit, p = lowest(m[idx])
        m[idx] &= ~bit
        acc = accept_single(prims[p], o[idx], d[idx], tmax[idx])
        hit[idx[acc]] = True; m[idx[acc]] = 0


# ---- the pair form -------------------------------------------------------------------------------------------------------------------
def boxes_pair(flat, o, dA, dB, tmaxA, tmaxB):
    s0 = flat[None, :, 0:3] - o[:, None, :]; s1 = flat[None, :, 4:7] - o[:, None, :]        # once per leaf
    bits = flat[:, 3].view(U)
    out = []
    for d, tmax in ((dA, tmaxA), (dB, tmaxB)):
        inv = rcp(d)
        out.append(to_mask(box_pass(s0 * inv[:, None, :], s1 * inv[:, None, :], tmax), bits))
    return out


def prims_pair(mA, mB, prims, o, dA, dB, tmaxA, tmaxB, gated=True):
    """flat_prims_pair -> (verdict A, verdict B, foreign): foreign counts the candidates that only the OTHER ray's mask holds and that would accept for an
    open ray.  gated=False: the loop without the own-mask gating (what the gating is there to prevent)."""
    mA = mA.copy(); mB = mB.copy(); todo = mA | mB
    hA = np.zeros(len(mA), bool); hB = np.zeros(len(mA), bool); foreign = 0
    while True:
        idx = np.nonzero(todo)[0]
        if not len(idx):
            return hA, hB, foreign
        bit, p = lowest(todo[idx])
        todo[idx] &= ~bit
        rec = prims[p]; oo = o[idx]
        n = rec[:, 12:15]
        oa = rec[:, 0:3] - oo
        noa = dot(n, oa)                                                              # once per candidate
        ob = rec[:, 4:7] - oo; oc = rec[:, 8:11] - oo
        tri = rec[:, 15].view(np.int32) == TRIANGLE
        v0 = cross(oc, ob); v1 = cross(ob, oa); v2t = cross(oa, oc)
        od = np.stack([rec[:, 3], rec[:, 7], rec[:, 11]], 1) - oo
        v2r = cross(oa, od); v3r = cross(od, oc)
        acc = []
        for m, other, d, tmax in ((mA, mB, dA, tmaxA), (mB, mA, dB, tmaxB)):
            dd = d[idx]
            dist = noa / dot(n, dd)
            ok = (dist > TMIN) & (dist < tmax[idx])
            ins = np.where(tri, same_sign([dot(v0, dd), dot(v1, dd), dot(v2t, dd)]), same_sign([dot(v0, dd), dot(v1, dd), dot(v2r, dd), dot(v3r, dd)]))
            own = (m[idx] & bit) != 0
            is_open = m[idx] != 0
            foreign += int((~own & is_open & ((other[idx] & bit) != 0) & ok & ins).sum())
            acc.append((own if gated else is_open) & ok & ins)
        hA[idx[acc[0]]] = True; mA[idx[acc[0]]] = 0
        hB[idx[acc[1]]] = True; mB[idx[acc[1]]] = 0
        todo[idx] &= mA[idx] | mB[idx]


def compare(flat, prims, o, dA, dB, tmaxA, tmaxB):
    """zero differences in both masks and both verdicts -> (occluded rays, foreign candidates that would have accepted, verdicts an ungated loop changes)"""
    occ = foreign = bites = 0
    for a in range(0, len(o), CHUNK):
        s = slice(a, a + CHUNK)
        with np.errstate(all="ignore"):
            m1A = boxes_single(flat, o[s], dA[s], tmaxA[s]); m1B = boxes_single(flat, o[s], dB[s], tmaxB[s])
            m2A, m2B = boxes_pair(flat, o[s], dA[s], dB[s], tmaxA[s], tmaxB[s])
            assert np.array_equal(m1A, m2A) and np.array_equal(m1B, m2B), "masks differ, first set %d" % (a + np.argmax((m1A != m2A) | (m1B != m2B)))
            h1A = prims_single(m1A, prims, o[s], dA[s], tmaxA[s]); h1B = prims_single(m1B, prims, o[s], dB[s], tmaxB[s])
            h2A, h2B, f = prims_pair(m2A, m2B, prims, o[s], dA[s], dB[s], tmaxA[s], tmaxB[s])
            assert np.array_equal(h1A, h2A) and np.array_equal(h1B, h2B), "verdicts differ, first set %d" % (a + np.argmax((h1A != h2A) | (h1B != h2B)))
            if f:
                uA, uB, _ = prims_pair(m2A, m2B, prims, o[s], dA[s], dB[s], tmaxA[s], tmaxB[s], gated=False)
                bites += int((uA != h1A).sum() + (uB != h1B).sum())
        occ += int(h1A.sum() + h1B.sum()); foreign += f
    return occ, foreign, bites


# ---- tables --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell():
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    sp = be.flatten()
    flat = jp.copy_upload_table(sp, "flat").view(F).reshape(-1, 8).copy()
    prims = jp.copy_upload_table(sp, "prims").view(F).reshape(-1, 16).copy()
    be.close()
    assert len(prims) == 32 and 2 <= len(flat) <= 32 and (prims[:, 15].view(np.int32) == TRIANGLE).all()
    assert np.bitwise_or.reduce(flat[:, 3].view(U)) == U(0xFFFFFFFF)                  # every primitive sits in some leaf
    return flat, prims


def random_table(seed, shrink=None):
    """20 triangles and 12 rectangles in leaves of two, records and leaf list laid out like the upload's.  shrink: the leaf boxes scaled about their centres
    (no longer bounding: for the foreign-bit cases only); None: padded bounding boxes like the upload's."""
    rng = np.random.default_rng(seed)
    prims = np.zeros((32, 16), F); corners = []
    for i in range(32):
        p0 = rng.uniform(0, 500, 3); e1 = rng.normal(0, 90, 3); e2 = rng.normal(0, 90, 3)
        if i % 4 == 0:                                                               # axis-aligned ones: origins can lie EXACTLY on their plane
            ax = rng.integers(0, 3); e1[ax] = 0; e2[ax] = 0; p0[ax] = np.round(p0[ax])
        if i < 20:
            pts = [p0, p0 + e1, p0 + e2]; kind = TRIANGLE
        else:
            e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
            pts = [p0, p0 + e1, p0 + e1 + e2, p0 + e2]; kind = RECTANGLE
        pts = [p.astype(F) for p in pts]
        n = np.cross((pts[1] - pts[0]).astype(np.float64), (pts[-1] - pts[0]).astype(np.float64)); n = (n / np.linalg.norm(n)).astype(F)
        prims[i, 0:3], prims[i, 4:7], prims[i, 8:11], prims[i, 12:15] = pts[0], pts[1], pts[2], n
        if kind == RECTANGLE:
            prims[i, 3], prims[i, 7], prims[i, 11] = pts[3]
        prims[i, 15:16].view(np.int32)[0] = kind
        corners.append(np.stack(pts))
    flat = np.zeros((16, 8), F)
    order = rng.permutation(32)
    for l in range(16):
        a, b = order[2 * l], order[2 * l + 1]
        pts = np.concatenate([corners[a], corners[b]])
        lo, hi = pts.min(0), pts.max(0)
        if shrink is not None:
            c = (lo + hi) / 2; lo = c + (lo - c) * shrink; hi = c + (hi - c) * shrink
        pad = F(1e-6) * np.maximum(np.abs(lo), np.abs(hi)) + F(1e-6)
        flat[l, 0:3] = np.nextafter((lo - pad).astype(F), F(-np.inf)); flat[l, 4:7] = np.nextafter((hi + pad).astype(F), F(np.inf))
        flat[l, 3:4].view(U)[0] = (U(1) << U(a)) | (U(1) << U(b))
    assert (flat[:, 0:3] < flat[:, 4:7]).all()
    return flat, prims


def points_on(prims, idx, rng):
    """a random point of primitive idx[k] each, in fp32"""
    u = rng.random(len(idx)); v = rng.random(len(idx))
    tri = prims[idx, 15].view(np.int32) == TRIANGLE
    fold = tri & (u + v > 1); u = np.where(fold, 1 - u, u); v = np.where(fold, 1 - v, v)
    p0 = prims[idx, 0:3]; p1 = prims[idx, 4:7]
    pl = np.where(tri[:, None], prims[idx, 8:11], np.stack([prims[idx, 3], prims[idx, 7], prims[idx, 11]], 1))    # the corner next to p0 on the other side
    return (p0 + (p1 - p0) * u[:, None].astype(F) + (pl - p0) * v[:, None].astype(F)).astype(F)


def aim(o, target):
    d = target - o
    dist = np.sqrt(dot(d, d)).astype(F)
    with np.errstate(all="ignore"):
        return (d / dist[:, None]).astype(F), dist


def tmax_kinds(rng, dist):
    """per set: both rays up to their targets; the same tmax for both; wildly different ones (1e-3 .. 1e6, +inf among them)"""
    n = len(dist[0])
    kind = rng.integers(0, 3, n)
    wild = [np.where(rng.random(n) < 0.1, np.inf, 10.0 ** rng.uniform(-3, 6, n)).astype(F) for _ in range(2)]
    tA = np.where(kind == 0, dist[0] - F(0.001), np.where(kind == 1, dist[0], wild[0])).astype(F)
    tB = np.where(kind == 0, dist[1] - F(0.001), np.where(kind == 1, dist[0], wild[1])).astype(F)
    return tA, tB


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
SETS = dict(cornell=420_000, random=160_000, adversarial=110_000, foreign=100_000)     # per test case; random, adversarial and foreign run twice each


def test_cornell_lamp_pairs(cornell):
    """origins on the box's own surfaces and in its interior, two rays each towards points of the two lamp triangles (primitives with the lamp's height)"""
    flat, prims = cornell
    rng = np.random.default_rng(1)
    n = SETS["cornell"]
    lamp = np.nonzero((np.abs(prims[:, [1, 5, 9]] - F(548.7)) < 0.01).all(1))[0]
    assert len(lamp) == 2
    o = points_on(prims, rng.integers(0, 32, n), rng)
    inside = rng.random(n) < 0.25
    o[inside] = np.stack([rng.uniform(1, 548, inside.sum()), rng.uniform(1, 548, inside.sum()), -rng.uniform(1, 558, inside.sum())], 1).astype(F)
    (dA, distA), (dB, distB) = (aim(o, points_on(prims, np.full(n, lamp[k]), rng)) for k in (0, 1))
    tA, tB = tmax_kinds(rng, (distA, distB))
    occ, _, _ = compare(flat, prims, o, dA, dB, tA, tB)
    assert n // 20 < occ < 2 * n                                       # some rays are shadowed by the boxes, most reach the lamp


@pytest.mark.parametrize("seed", [11, 12])
def test_random_tables(seed):
    flat, prims = random_table(seed)
    rng = np.random.default_rng(seed + 100)
    n = SETS["random"]
    o = rng.uniform(-50, 550, (n, 3)).astype(F)
    half = n // 2                                                      # half of the sets aim at primitives, the others anywhere
    tgtA = np.where((np.arange(n) < half)[:, None], points_on(prims, rng.integers(0, 32, n), rng), rng.uniform(-50, 550, (n, 3))).astype(F)
    tgtB = np.where((np.arange(n) < half)[:, None], points_on(prims, rng.integers(0, 32, n), rng), rng.uniform(-50, 550, (n, 3))).astype(F)
    (dA, distA), (dB, distB) = aim(o, tgtA), aim(o, tgtB)
    tA, tB = tmax_kinds(rng, (distA * F(1.5), distB * F(1.5)))
    occ, _, _ = compare(flat, prims, o, dA, dB, tA, tB)
    assert occ > n // 20


@pytest.mark.parametrize("table", ["cornell", "random"])
def test_adversarial_sets(cornell, table):
    """origins exactly on a primitive's plane (a point of the primitive; exact for the axis-aligned ones) or on a padded box plane; direction components
    0, -0, denormal and +-tiny next to ordinary ones, up to all three at once"""
    flat, prims = cornell if table == "cornell" else random_table(13)
    rng = np.random.default_rng(21)
    n = SETS["adversarial"]
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, TINY, -TINY, 1e-30, -1e-30, 1.0, -1.0], F)
    which = rng.integers(0, len(prims), n)
    o = points_on(prims, which, rng)
    exact = int((dot(prims[which, 12:15], prims[which, 0:3] - o) == 0).sum())         # dot(n, oa) == 0: the plane distance of the own primitive is exactly 0
    b = rng.integers(0, len(flat), (n, 3)); side = rng.integers(0, 2, (n, 3)) * 4
    o = np.where(rng.random((n, 3)) < 0.3, flat[b, side + np.arange(3)[None, :]], o).astype(F)
    ds = []
    for _ in range(2):
        d, _ = aim(o, points_on(prims, rng.integers(0, len(prims), n), rng))
        d = np.where(rng.random((n, 3)) < 0.4, special[rng.integers(0, len(special), (n, 3))], d).astype(F)
        d[: n // 16] = special[rng.integers(0, 6, (n // 16, 3))]
        ds.append(d)
    tA, tB = tmax_kinds(rng, (np.full(n, 300.0, F), np.full(n, 700.0, F)))
    compare(flat, prims, o, ds[0], ds[1], tA, tB)
    assert exact > n // 50, exact                                      # the axis-aligned primitives give origins exactly on a plane


def test_foreign_bits_are_never_counted():
    """leaf boxes shrunk to 45 % about their centres: ray B aims at a primitive through its leaf's shrunken box, ray A at the same primitive's rim, past the
    box.  The primitive then lies in mB only and the triangle / rectangle test accepts it for ray A: the sequential walk never tests it for A, so the pair
    loop must not count it either.  The number of such candidates is printed and must be above zero; so must the number of verdicts a pair loop WITHOUT
    the own-mask gating gets wrong on the same sets, otherwise this test would not see the gating."""
    total = foreign = bites = 0
    for seed in (31, 32):
        flat, prims = random_table(seed, shrink=0.45)
        rng = np.random.default_rng(seed + 100)
        n = SETS["foreign"]
        o = rng.uniform(-50, 550, (n, 3)).astype(F)
        which = rng.integers(0, 32, n)
        (dA, distA), (dB, distB) = aim(o, points_on(prims, which, rng)), aim(o, points_on(prims, which, rng))
        tA, tB = tmax_kinds(rng, (distA * F(1.5), distB * F(1.5)))
        _, f, w = compare(flat, prims, o, dA, dB, tA, tB)
        total += n; foreign += f; bites += w
    print("foreign-bit cases: %d candidates in the other ray's mask only that would accept, over %d sets; an ungated loop changes %d verdicts" % (foreign, total, bites))
    assert foreign > 1000 and bites > 1000


def test_at_least_a_million_sets():
    assert SETS["cornell"] + 2 * (SETS["random"] + SETS["adversarial"] + SETS["foreign"]) >= 1_000_000
