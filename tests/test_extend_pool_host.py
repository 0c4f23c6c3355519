"""The pooled closest-hit pass (csrc/jp_device.h: flat_prims_pool; DESIGN.md section 5, "Pooled closest hits") against the loop it replaces, as float32
numpy models of both forms.  No GPU needed.

  sequential   flat_prims<closest hit>: the ray's own mask in __ffs order, tri_hit / rect_hit against the SHRINKING tmax (an accepted hit becomes the
               new tmax), the last accepted candidate is the hit
  pooled       every candidate of the ray's mask against the ray's ORIGINAL tmax (k_extend: +inf); the hit is the minimum of
               (distance bits << 32 | primitive) over the accepted ones, as the 64-bit LDS atomic min leaves it
  wrong rule   the pooled form with the HIGHEST index winning among equal distances: what a wrong key would compute.  The tie cases assert that it
               differs from the sequential loop there, so the comparison cannot pass vacuously.

Every operation is one IEEE fp32 operation in tri_hit's / rect_hit's order, as under -ffp-contract=off.  Expected: zero differences in
(primitive, distance bits) -- over the Cornell tables, random triangle / rectangle tables, tables with duplicated and coplanar primitives (exact distance
ties), origins exactly on primitive planes (dot(n, oa) == 0), directions in a primitive's plane (dot(n, d) == 0: the quotient is inf or NaN), direction
components 0, -0 and denormal, and hits at exactly tmin.  test_ring_serves_every_pair_once walks the list bookkeeping of flat_prims_pool (ballot ranks, the
128-entry ring, a dense round as soon as 64 entries wait) with integers: every (lane, primitive) pair is tested exactly once and no unread entry is
overwritten."""
import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

F = np.float32
U = np.uint32
TINY = np.finfo(F).tiny
SLACK = F(1.000002)
TRIANGLE, RECTANGLE = 0, 1                      # JP_SHAPE_* (include/jetpbrt_amd.h)
CHUNK = 1 << 16
MISS = np.int64(-1)

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


def box_masks(flat, o, d, tmin, tmax):
    """flat_boxes_lean<false> (with tmax = +inf: flat_boxes_lean<true>, whose mask is the same bits) -> the candidate mask per ray"""
    inv = rcp(d)
    t0 = (flat[None, :, 0:3] - o[:, None, :]) * inv[:, None, :]
    t1 = (flat[None, :, 4:7] - o[:, None, :]) * inv[:, None, :]
    n, f = np.fmin(t0, t1), np.fmax(t0, t1)
    tn = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], tmin[:, None]))
    tf = np.fmin(np.fmin(f[..., 0], f[..., 1]), np.fmin(f[..., 2], tmax[:, None]))
    return np.bitwise_or.reduce(np.where(tn <= tf * SLACK, flat[:, 3].view(U)[None, :], U(0)), axis=1).astype(U)


def accept(rec, o, d, tmin, tmax):
    """prim_hit<FeatFlat>: tri_hit / rect_hit on the records rec (K, 16) -> (accepted, distance)"""
    n = rec[:, 12:15]
    oa = rec[:, 0:3] - o
    dist = (dot(n, oa) / dot(n, d)).astype(F)
    ok = (dist > tmin) & (dist < tmax)
    ob = rec[:, 4:7] - o; oc = rec[:, 8:11] - o
    tri = rec[:, 15].view(np.int32) == TRIANGLE
    v0 = cross(oc, ob); v1 = cross(ob, oa)
    v2t = cross(oa, oc)
    od = np.stack([rec[:, 3], rec[:, 7], rec[:, 11]], 1) - o
    v2r = cross(oa, od); v3r = cross(od, oc)
    in_t = same_sign([dot(v0, d), dot(v1, d), dot(v2t, d)])
    in_r = same_sign([dot(v0, d), dot(v1, d), dot(v2r, d), dot(v3r, d)])
    return ok & np.where(tri, in_t, in_r), dist


def lowest(m):
    bit = (m & (~m + U(1))).astype(U)
    return bit, np.log2(bit.astype(np.float64)).astype(np.int64)


# ---- the two forms -------------------------------------------------------------------------------------------------------------------
def sequential(mask, prims, o, d, tmin, tmax0):
    """flat_prims<false, false>: -> (primitive or -1, bits of tmax on return)"""
    m = mask.copy(); tmax = tmax0.copy(); hit = np.full(len(m), MISS)
    while True:
        idx = np.nonzero(m)[0]
        if not len(idx):
            return hit, tmax.view(U).copy()
        bit, p = lowest(m[idx])
        m[idx] &= ~bit
        acc, dist = accept(prims[p], o[idx], d[idx], tmin[idx], tmax[idx])
        tmax[idx[acc]] = dist[acc]; hit[idx[acc]] = p[acc]


def pooled(mask, prims, o, d, tmin, tmax0, highest_index_wins=False):
    """flat_prims_pool: the minimum of the 64-bit keys of the accepted candidates, in whatever order they arrive -> (primitive or -1, bits of tmax on return)"""
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(len(mask), none)
    for p in np.random.default_rng(5).permutation(len(prims)):                          # any order: a minimum does not depend on it
        idx = np.nonzero(mask & (U(1) << U(p)))[0]
        if not len(idx):
            continue
        acc, dist = accept(prims[np.full(len(idx), p)], o[idx], d[idx], tmin[idx], tmax0[idx])
        low = np.uint64(31 - p if highest_index_wins else p)
        key = (dist.view(U).astype(np.uint64) << np.uint64(32)) | low
        best[idx[acc]] = np.minimum(best[idx[acc]], key[acc])
    found = best != none
    low = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit = np.where(found, 31 - low if highest_index_wins else low, MISS)
    t = np.where(found, (best >> np.uint64(32)).astype(U), tmax0.view(U))
    return hit, t.astype(U)


def compare(flat, prims, o, d, tmin=None, tmax=None, masks=None):
    """zero differences between the two forms -> (hits, rays where the wrong tie rule gives another record)"""
    n = len(o)
    tmin = np.full(n, 0.001, F) if tmin is None else tmin.astype(F)
    tmax = np.full(n, np.inf, F) if tmax is None else tmax.astype(F)
    hits = wrong = 0
    for a in range(0, n, CHUNK):
        s = slice(a, a + CHUNK)
        with np.errstate(all="ignore"):
            m = box_masks(flat, o[s], d[s], tmin[s], tmax[s]) if masks is None else masks[s]
            h1, t1 = sequential(m, prims, o[s], d[s], tmin[s], tmax[s])
            h2, t2 = pooled(m, prims, o[s], d[s], tmin[s], tmax[s])
            h3, t3 = pooled(m, prims, o[s], d[s], tmin[s], tmax[s], highest_index_wins=True)
        bad = (h1 != h2) | (t1 != t2)
        assert not bad.any(), "%d records differ, first ray %d: sequential (%d, %08x) pooled (%d, %08x)" % (bad.sum(), a + np.argmax(bad), h1[np.argmax(bad)], t1[np.argmax(bad)],
                                                                                                          h2[np.argmax(bad)], t2[np.argmax(bad)])
        assert ((h1 >= 0) | (t1 == tmax[s].view(U))).all()                             # a miss leaves tmax as it came
        hits += int((h1 >= 0).sum()); wrong += int(((h1 != h3) | (t1 != t3)).sum())
    return hits, wrong


# ---- tables --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell():
    be = scenes.build_cornell(scenes.HostBackend("cornell"), 64, 64, lambert_only=False)
    sp = be.flatten()
    flat = jp.copy_upload_table(sp, "flat").view(F).reshape(-1, 8).copy()
    prims = jp.copy_upload_table(sp, "prims").view(F).reshape(-1, 16).copy()
    be.close()
    assert len(prims) == 32 and 2 <= len(flat) <= 32 and (prims[:, 15].view(np.int32) == TRIANGLE).all()
    return flat, prims


def leaves_of(corners, groups):
    """padded bounding boxes like the upload's, one leaf per group of primitive indices"""
    flat = np.zeros((len(groups), 8), F)
    for l, g in enumerate(groups):
        pts = np.concatenate([corners[i] for i in g])
        lo, hi = pts.min(0), pts.max(0)
        pad = F(1e-6) * np.maximum(np.abs(lo), np.abs(hi)) + F(1e-6)
        flat[l, 0:3] = np.nextafter((lo - pad).astype(F), F(-np.inf)); flat[l, 4:7] = np.nextafter((hi + pad).astype(F), F(np.inf))
        bits = U(0)
        for i in g:
            bits |= U(1) << U(i)
        flat[l, 3:4].view(U)[0] = bits
    assert (flat[:, 0:3] < flat[:, 4:7]).all()
    return flat


def random_table(seed, n_prims=32, duplicates=False):
    """triangles and rectangles, every fourth one axis-aligned at integer coordinates (origins can lie EXACTLY on its plane, directions exactly in it).
    duplicates: the upper half of the table repeats the lower half -- primitive i + 16 is primitive i, or (every other one) the rest of its plane's
    parallelogram: a coplanar neighbour with the same p0 and normal, so the plane distances of the two are the same bits"""
    rng = np.random.default_rng(seed)
    prims = np.zeros((n_prims, 16), F); corners = []
    for i in range(n_prims):
        if duplicates and i >= n_prims // 2:
            j = i - n_prims // 2
            prims[i] = prims[j]; pts = [c.copy() for c in corners[j]]
            if j % 2 and prims[j, 15:16].view(np.int32)[0] == TRIANGLE:
                pts = [pts[0], (pts[1] + pts[2] - pts[0]).astype(F), pts[2]]            # p0, p1 + p2 - p0, p2: the other half of the parallelogram, p0 and n kept
                prims[i, 4:7] = pts[1]
            corners.append(np.stack(pts))
            continue
        p0 = rng.uniform(0, 500, 3); e1 = rng.normal(0, 90, 3); e2 = rng.normal(0, 90, 3)
        if i % 4 == 0:
            ax = rng.integers(0, 3); e1[ax] = 0; e2[ax] = 0; p0 = np.round(p0); e1 = np.round(e1); e2 = np.round(e2)
            if not np.cross(e1, e2).any():
                e1 = np.roll(np.eye(3)[ax], 1) * 40; e2 = np.roll(np.eye(3)[ax], 2) * 30
        if i % 8 < 5:
            pts = [p0, p0 + e1, p0 + e2]; kind = TRIANGLE
        else:
            if i % 4:
                e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
            pts = [p0, p0 + e1, p0 + e1 + e2, p0 + e2]; kind = RECTANGLE
        pts = [p.astype(F) for p in pts]
        n = np.cross((pts[1] - pts[0]).astype(np.float64), (pts[-1] - pts[0]).astype(np.float64)); n = (n / np.linalg.norm(n)).astype(F)
        prims[i, 0:3], prims[i, 4:7], prims[i, 8:11], prims[i, 12:15] = pts[0], pts[1], pts[2], n
        if kind == RECTANGLE:
            prims[i, 3], prims[i, 7], prims[i, 11] = pts[3]
        prims[i, 15:16].view(np.int32)[0] = kind
        corners.append(np.stack(pts))
    half = n_prims // 2
    groups = [(i, i + half) for i in range(half)] if duplicates else [tuple(g) for g in rng.permutation(n_prims).reshape(-1, 2)]
    return leaves_of(corners, groups), prims


def points_on(prims, idx, rng):
    """a random point of primitive idx[k] each, in fp32"""
    u = rng.random(len(idx)); v = rng.random(len(idx))
    tri = prims[idx, 15].view(np.int32) == TRIANGLE
    fold = tri & (u + v > 1); u = np.where(fold, 1 - u, u); v = np.where(fold, 1 - v, v)
    p0 = prims[idx, 0:3]; p1 = prims[idx, 4:7]
    pl = np.where(tri[:, None], prims[idx, 8:11], np.stack([prims[idx, 3], prims[idx, 7], prims[idx, 11]], 1))
    return (p0 + (p1 - p0) * u[:, None].astype(F) + (pl - p0) * v[:, None].astype(F)).astype(F)


def aim(o, target):
    d = target - o
    with np.errstate(all="ignore"):
        return (d / np.sqrt(dot(d, d)).astype(F)[:, None]).astype(F)


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, TINY, -TINY, 1e-30, -1e-30, 1.0, -1.0], F)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def test_cornell_rays(cornell):
    """origins on the box's own surfaces (bounce rays) and in its interior, directions towards other surface points and anywhere"""
    flat, prims = cornell
    rng = np.random.default_rng(1)
    n = 300_000
    o = points_on(prims, rng.integers(0, 32, n), rng)
    inside = rng.random(n) < 0.3
    o[inside] = np.stack([rng.uniform(1, 548, inside.sum()), rng.uniform(1, 548, inside.sum()), -rng.uniform(1, 558, inside.sum())], 1).astype(F)
    d = aim(o, points_on(prims, rng.integers(0, 32, n), rng))
    anyw = rng.normal(size=(n, 3)); anyw = (anyw / np.linalg.norm(anyw, axis=1, keepdims=True)).astype(F)
    d = np.where((rng.random(n) < 0.5)[:, None], anyw, d).astype(F)
    hits, _ = compare(flat, prims, o, d)
    assert hits > n // 2


@pytest.mark.parametrize("seed", [11, 12])
def test_random_tables(seed):
    flat, prims = random_table(seed)
    rng = np.random.default_rng(seed + 100)
    n = 150_000
    o = rng.uniform(-50, 550, (n, 3)).astype(F)
    d = aim(o, np.where((np.arange(n) < n // 2)[:, None], points_on(prims, rng.integers(0, 32, n), rng), rng.uniform(-50, 550, (n, 3))).astype(F))
    tmax = np.where(rng.random(n) < 0.5, np.inf, 10.0 ** rng.uniform(-3, 4, n)).astype(F)                     # jp_trace's rays carry their own far ends
    tmin = np.where(rng.random(n) < 0.5, 0.001, 10.0 ** rng.uniform(-4, 2, n)).astype(F)
    hits, _ = compare(flat, prims, o, d, tmin, tmax)
    assert hits > n // 20


@pytest.mark.parametrize("seed", [21, 22])
def test_exact_distance_ties(seed):
    """primitive i + 16 repeats primitive i or completes its parallelogram (same p0, same normal: the same distance bits), both in one leaf.  Rays aimed at
    the lower half's primitives: the sequential loop keeps the FIRST of the equal distances (`distance < tmax` is strict), so must the pooled key; the
    wrong rule must give another record on these rays, and with every candidate forced into every mask too"""
    flat, prims = random_table(seed, duplicates=True)
    rng = np.random.default_rng(seed + 100)
    n = 100_000
    o = rng.uniform(-50, 550, (n, 3)).astype(F)
    d = aim(o, points_on(prims, rng.integers(0, 16, n), rng))
    hits, wrong = compare(flat, prims, o, d)
    assert hits > n // 2 and wrong > n // 8, (hits, wrong)
    hits, wrong = compare(flat, prims, o, d, masks=np.full(n, 0xFFFFFFFF, U))
    assert hits > n // 2 and wrong > n // 8, (hits, wrong)


def test_constructed_ties():
    """two identical triangles at indices 3 and 17 and a nearer, a farther and a missed one around them, every bit set: the answer is index 3 with the
    shared distance; listed by hand so that the expected record is known without either model"""
    tri = lambda z, s=100.0: [(-s, -s, z), (s, -s, z), (0.0, s, z)]
    prims = np.zeros((32, 16), F)
    for i in range(32):
        pts = tri(-900.0 - i) if i not in (3, 17, 9) else tri(-50.0)                    # far planes behind; 3 and 17 the same triangle; 9 coplanar with them ...
        if i == 9:
            pts = [(300.0, 300.0, -50.0), (400.0, 300.0, -50.0), (350.0, 400.0, -50.0)]   # ... but off to the side: same distance bits, inside test fails
        prims[i, 0:3], prims[i, 4:7], prims[i, 8:11] = pts
        prims[i, 12:15] = (0, 0, 1)
    o = np.array([[0.0, 0.0, 0.0], [1.0, -2.0, 10.0]], F); d = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]], F)
    mask = np.full(2, 0xFFFFFFFF, U); tmin = np.full(2, 0.001, F); tmax = np.full(2, np.inf, F)
    for form in (sequential, pooled):
        h, t = form(mask, prims, o, d, tmin, tmax)
        assert h.tolist() == [3, 3] and t.view(F).tolist() == [50.0, 60.0], (form.__name__, h, t.view(F))
    h, _ = pooled(mask, prims, o, d, tmin, tmax, highest_index_wins=True)
    assert h.tolist() == [17, 17]


@pytest.mark.parametrize("table", ["cornell", "random", "ties"])
def test_adversarial_sets(cornell, table):
    """origins exactly on a primitive's plane (dot(n, oa) == 0 for the axis-aligned ones: the quotient is 0 or, with the direction in the plane too, NaN);
    directions in a primitive's plane (dot(n, d) == 0: +-inf); direction components 0, -0, denormal and +-tiny, up to all three at once"""
    flat, prims = cornell if table == "cornell" else random_table(13, duplicates=table == "ties")
    rng = np.random.default_rng(31)
    n = 120_000
    which = rng.integers(0, len(prims), n)
    o = points_on(prims, which, rng)
    on_plane = dot(prims[which, 12:15], prims[which, 0:3] - o) == 0
    b = rng.integers(0, len(flat), (n, 3)); side = rng.integers(0, 2, (n, 3)) * 4
    o = np.where(rng.random((n, 3)) < 0.2, flat[b, side + np.arange(3)[None, :]], o).astype(F)
    d = aim(o, points_on(prims, rng.integers(0, len(prims), n), rng))
    d = np.where(rng.random((n, 3)) < 0.4, SPECIAL[rng.integers(0, len(SPECIAL), (n, 3))], d).astype(F)
    d[: n // 16] = SPECIAL[rng.integers(0, 6, (n // 16, 3))]
    other = rng.integers(0, len(prims), n)                              # a quarter of the rays: the direction exactly in another primitive's plane where that is axis-aligned
    nrm = prims[other, 12:15]
    flatten = (rng.random(n) < 0.25)[:, None] & (np.abs(nrm) == 1)
    d = np.where(flatten, F(0) * np.where(rng.random((n, 3)) < 0.5, -1, 1), d).astype(F)
    in_plane = dot(nrm, d) == 0
    with np.errstate(all="ignore"):
        q = dot(prims[which, 12:15], prims[which, 0:3] - o) / dot(prims[which, 12:15], d)
    assert on_plane.sum() > n // 50 and in_plane.sum() > n // 50 and np.isnan(q).sum() > 100 and np.isinf(q).sum() > 100, (on_plane.sum(), in_plane.sum(), np.isnan(q).sum(), np.isinf(q).sum())
    compare(flat, prims, o, d)
    compare(flat, prims, o, d, masks=np.full(n, (1 << len(prims)) - 1 if len(prims) < 32 else 0xFFFFFFFF, U))   # and with every candidate in every mask


def test_hits_at_exactly_tmin():
    """axis-aligned primitives at integer coordinates, origins a power of two in front of them along the normal: the plane distance is exactly that
    number.  tmin equal to it rejects (`distance > tmin` is strict), one ulp below accepts -- in both forms"""
    flat, prims = random_table(41)
    rng = np.random.default_rng(42)
    axis_aligned = np.nonzero((np.abs(prims[:, 12:15]) == 1).any(1))[0]
    assert len(axis_aligned) >= 8
    n = 60_000
    which = axis_aligned[rng.integers(0, len(axis_aligned), n)]
    h = (2.0 ** rng.integers(-6, 5, n)).astype(F)
    nrm = prims[which, 12:15]
    o = (points_on(prims, which, rng) + nrm * h[:, None]).astype(F)
    d = (-nrm).astype(F)
    with np.errstate(all="ignore"):
        dist = (dot(nrm, prims[which, 0:3] - o) / dot(nrm, d)).astype(F)
    assert (dist == h).mean() > 0.9                                     # the construction is exact for almost every ray
    kind = rng.integers(0, 3, n)
    tmin = np.where(kind == 0, h, np.where(kind == 1, np.nextafter(h, F(0)), np.nextafter(h, F(np.inf)))).astype(F)
    every = np.full(n, 0xFFFFFFFF, U)
    hits, _ = compare(flat, prims, o, d, tmin=tmin, masks=every)
    with np.errstate(all="ignore"):
        hs, ts = sequential(every, prims, o, d, tmin, np.full(n, np.inf, F))
    exact = dist == h
    assert not ((kind == 0) & exact & (hs == which)).any()              # at exactly tmin: never that primitive at that distance
    assert ((kind == 1) & exact & (ts.view(F) == h)).sum() > n // 8      # one ulp below: accepted at exactly h (where the random point passes the inside test)


def test_ring_serves_every_pair_once():
    """the list bookkeeping of flat_prims_pool with integers: per trip the lanes that hold a candidate append (lane << 8 | lowest set bit) at
    (tail + ballot rank) & 127, a round takes 64 entries from head as soon as 64 wait, a last round takes the rest"""
    rng = np.random.default_rng(7)
    for case in range(400):
        dens = rng.choice([0.0, 0.03, 0.1, 0.3, 0.7, 1.0])
        masks = np.array([int(rng.integers(0, 1 << 32)) if rng.random() < 0.9 else 0xFFFFFFFF for _ in range(64)], np.uint64)
        masks &= np.array([sum(1 << b for b in range(32) if rng.random() < dens) for _ in range(64)], np.uint64)
        if case % 7 == 0:
            masks[rng.integers(0, 64)] = 0xFFFFFFFF                        # one full lane among sparse ones
        want = sorted((l, b) for l in range(64) for b in range(32) if (int(masks[l]) >> b) & 1)
        ring = [None] * 128; head = tail = 0; seen = []; rounds = 0
        m = [int(x) for x in masks]

        def dense(k):
            nonlocal head, rounds
            for lane in range(k):
                e = ring[(head + lane) & 127]
                assert e is not None
                seen.append((e >> 8, e & 0xFF)); ring[(head + lane) & 127] = None
            head += k; rounds += 1
        trips = 0
        while any(m):
            live = [l for l in range(64) if m[l]]
            assert tail - head < 64
            for rank, l in enumerate(live):
                pos = (tail + rank) & 127
                assert ring[pos] is None, "an entry that waits was overwritten"
                ring[pos] = (l << 8) | ((m[l] & -m[l]).bit_length() - 1)
                m[l] &= m[l] - 1
            tail += len(live); trips += 1
            if tail - head >= 64:
                dense(64)
        if tail != head:
            dense(tail - head)
        assert sorted(seen) == want and trips == max(bin(int(x)).count("1") for x in masks) and rounds == (len(want) + 63) // 64
