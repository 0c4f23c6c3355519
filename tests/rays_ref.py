"""A float64 ray caster for the per-ray tests of the traversal (tests/test_rays_host.py, tests/test_gpu_occluded.py), written from the shape definitions:
a triangle and a rectangle are the convex polygon through their corners, a disk is the points of its plane within `r` of its centre, a sphere the points at
`r` from its centre; a ray (o, d, tmin, tmax) hits a shape at a parameter t with tmin < t < tmax.  Nothing here follows the device code or the oracle: no
boxes, no tree, no fp32.  The tests compare the library and the fp32 oracle against this file.

Besides the nearest hit, `cast` says for every ray whether it is DECISIVE: no primitive is a close call for it -- or one primitive blocks it that is none,
whatever the others are -- so every valid fp32 evaluation must reach the float64 verdict.  With S the diagonal of the scene's bounding box, m = M_REL * S and, at a crossing t, m' = m * max(1, t / S), a primitive is a close
call for a ray when the ray
  * crosses its plane (or meets the sphere) at a t within m' of tmin or of tmax, at a point within m of the shape,
  * crosses its plane within m of the shape's boundary (polygon edge, disk rim) or passes the sphere's centre at a distance within m of r (in terms of the
    discriminant: |b^2 - c| within m (2 r + m)), at a t inside (tmin - m', tmax + m'),
  * meets the plane at a grazing angle, |cos| < GRAZING, and stays within m of the plane anywhere within m of the shape: over the stretch m / |cos| either
    side of the crossing (a ray parallel to the plane: anywhere, if it runs within m of the plane).
The first rule counts a plane crossing only where it lies within m of the shape: a crossing far outside the polygon is no hit under any rounding, and with
thousands of planes per scene a rule without that restriction would call every ray of a long far end a close call.
A zero component in d needs no special case: the planes are tested by division, and a ray parallel to a plane is decided by its distance from it.

The constants below are not tuned to the device.  tests/test_rays_host.py holds the fp32 CPU oracle (jp_oracle_trace; oracle/pt_oracle.cc, independent of the
device code and pinned to the reference) to the float64 verdict on every decisive ray of every scene and ray set of tests/rays_sets.py and measures its
distance error.  M_REL and GRAZING are starting values, to be widened by powers of ten until the oracle agrees everywhere; it agrees at the starting values."""
import numpy as np

TRIANGLE, RECTANGLE, SPHERE, DISK = 0, 1, 2, 3

# the margin, relative to the scene's diagonal, and the grazing bound: the oracle agrees with the float64 verdict on all decisive rays at these starting
# values (test_rays_host.py asserts it: 351,209 rays in 86 sets of 14 scenes, 316,554 decisive, no disagreement; nothing had to be widened)
M_REL = 1e-5
GRAZING = 0.05
# the oracle's worst |t_oracle - t_float64| / max(|t|, S) over the decisive hit rays of all sets (test_rays_host.py prints it per scene and asserts it stays below
# this figure), and the tolerance the GPU's closest-hit distance gets: four times that, headroom for another valid fp32 evaluation order.  No GPU result enters.
# Per shape class: a sphere's roots come from b^2 - c, which cancels in fp32 where the origin is far from a small sphere; a flat shape's t is one division.
# Measured: flat 2.30e-7 (one_disk, random), sphere 5.97e-6 (misc, shadow8); recorded rounded up.
ORACLE_T_WORST = {"flat": 2.4e-7, "sphere": 6.0e-6}
T_TOL = {k: 4 * v for k, v in ORACLE_T_WORST.items()}
MAX_NON_DECISIVE = 0.02               # cap on the share of non-decisive rays of any set (rays_sets.capped: all but the sets made of close calls on purpose)


def shape_class(sh, prim):
    """ "flat" / "sphere" per primitive index (for T_TOL)"""
    return np.where(sh.kind[prim] == SPHERE, "sphere", "flat")


# ---- the scene as the library receives it ---------------------------------------------------------------------------------------------------
def _arr(ptr, n, k=3):
    if n == 0:
        return np.zeros((0, k) if k > 1 else (0,), np.float64)
    a = np.ctypeslib.as_array(ptr, shape=(n * k,)).astype(np.float64)
    return a.reshape(n, k) if k > 1 else a


class Shapes:
    """the primitives of a flattened scene (JpScene) by kind, float64: polygons (triangles and rectangles together, 3 or 4 corners), spheres, disks; each
    with the caller's primitive index and its light (-1: none)"""

    def __init__(self, s):
        n = s.n_primitives
        kind = np.ctypeslib.as_array(s.prim_shape_type, shape=(n,)).copy()
        idx = np.ctypeslib.as_array(s.prim_shape_index, shape=(n,)).copy()
        self.light = np.ctypeslib.as_array(s.prim_light, shape=(n,)).copy()
        self.kind = kind
        self.n_prims = n
        tp = [_arr(p, s.n_triangles) for p in (s.tri_p0, s.tri_p1, s.tri_p2)]
        rp = [_arr(p, s.n_rectangles) for p in (s.rect_p0, s.rect_p1, s.rect_p2, s.rect_p3)]
        ti, ri = np.nonzero(kind == TRIANGLE)[0], np.nonzero(kind == RECTANGLE)[0]
        si, di = np.nonzero(kind == SPHERE)[0], np.nonzero(kind == DISK)[0]
        self.tri_prim, self.tri_v = ti, np.stack([p[idx[ti]] for p in tp], 1)            # (T, 3, 3)
        self.rect_prim, self.rect_v = ri, np.stack([p[idx[ri]] for p in rp], 1)          # (R, 4, 3): the corners in order round the rectangle
        self.sph_prim, self.sph_c, self.sph_r = si, _arr(s.sph_center, s.n_spheres)[idx[si]], _arr(s.sph_radius, s.n_spheres, 1)[idx[si]]
        self.disk_prim = di
        self.disk_c, self.disk_r = _arr(s.disk_center, s.n_disks)[idx[di]], _arr(s.disk_radius, s.n_disks, 1)[idx[di]]
        dn = _arr(s.disk_normal, s.n_disks)[idx[di]]
        self.disk_n = dn / np.linalg.norm(dn, axis=1, keepdims=True) if len(di) else dn
        self._finish()

    @classmethod
    def from_triangles(cls, v):
        """a scene of triangles alone, corners v (T, 3, 3)"""
        sh = cls.__new__(cls)
        T = len(v)
        sh.kind = np.zeros(T, np.int32); sh.light = np.full(T, -1); sh.n_prims = T
        sh.tri_prim, sh.tri_v = np.arange(T), np.asarray(v, np.float64)
        sh.rect_prim, sh.rect_v = np.zeros(0, np.int64), np.zeros((0, 4, 3))
        sh.sph_prim, sh.sph_c, sh.sph_r = np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros(0)
        sh.disk_prim, sh.disk_c, sh.disk_r, sh.disk_n = np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3))
        sh._finish()
        return sh

    def _finish(self):
        lo, hi = [], []
        for v in (self.tri_v.reshape(-1, 3), self.rect_v.reshape(-1, 3)):
            if len(v): lo.append(v.min(0)); hi.append(v.max(0))
        for c, r in ((self.sph_c, self.sph_r), (self.disk_c, self.disk_r)):
            if len(c): lo.append((c - r[:, None]).min(0)); hi.append((c + r[:, None]).max(0))
        self.lo, self.hi = np.min(lo, 0), np.max(hi, 0)
        self.S = float(np.linalg.norm(self.hi - self.lo))
        self.m = M_REL * self.S
        self._polys = [self._poly(self.tri_v, self.tri_prim), self._poly(self.rect_v, self.rect_prim)]

    @staticmethod
    def _poly(v, prim):
        """plane (unit normal n, offset k: n.x = k) and, per edge, the in-plane unit vector w pointing inward and its offset: the signed distance of a point x
        of the plane from the edge's line is w.x - kw, positive inside"""
        if len(v) == 0:
            return None
        K = v.shape[1]
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        cen = v.mean(1)
        W, KW = [], []
        for e in range(K):
            a, b = v[:, e], v[:, (e + 1) % K]
            w = np.cross(n, b - a)
            w /= np.linalg.norm(w, axis=1, keepdims=True)
            w *= np.sign(((cen - a) * w).sum(1))[:, None]
            W.append(w); KW.append((a * w).sum(1))
        return dict(prim=prim, n=n, k=(v[:, 0] * n).sum(1), W=W, KW=KW, centre=cen, radius=np.linalg.norm(v - cen[:, None, :], axis=2).max(1))


# ---- the caster -------------------------------------------------------------------------------------------------------------------------------
class _Best:
    """nearest and second-nearest hit per ray, and the close-call flag, gathered from (ray, primitive) pairs"""

    def __init__(self, n):
        self.n = n
        self.t1 = np.full(n, np.inf); self.t2 = np.full(n, np.inf); self.prim = np.full(n, -1, np.int64)
        self.close = np.zeros(n, bool); self.blocked = np.zeros(n, bool)

    def add(self, ri, t, hit, close, prim):
        """ri: the pair's ray; t, hit, close, prim: per pair"""
        self.close |= np.bincount(ri[close], minlength=self.n) > 0
        self.blocked |= np.bincount(ri[hit & ~close], minlength=self.n) > 0
        r, th, pr = ri[hit], t[hit], prim[hit]
        if len(r) == 0:
            return
        order = np.lexsort((th, r))
        r, th, pr = r[order], th[order], pr[order]
        first = np.nonzero(np.r_[True, r[1:] != r[:-1]])[0]
        a1 = np.full(self.n, np.inf); a2 = np.full(self.n, np.inf); ap = np.full(self.n, -1, np.int64)
        a1[r[first]] = th[first]; ap[r[first]] = pr[first]
        nxt = first + 1
        has = nxt < len(r)
        has[has] = r[nxt[has]] == r[first[has]]
        a2[r[first[has]]] = th[nxt[has]]
        nearer = a1 < self.t1
        self.t2 = np.where(nearer, np.minimum(self.t1, a2), np.minimum(self.t2, a1))
        self.prim = np.where(nearer, ap, self.prim)
        self.t1 = np.where(nearer, a1, self.t1)


def _pairs(o, du, centre, radius, m):
    """the (ray, primitive) pairs whose line comes within radius + 4 m of the primitive's centre: every hit and every close call is among them"""
    oc2 = (o * o).sum(1)[:, None] - 2.0 * (o @ centre.T) + (centre * centre).sum(1)[None, :]
    b = (o * du).sum(1)[:, None] - du @ centre.T                        # (o - c) . d
    return np.nonzero(oc2 - b * b <= (radius[None, :] + 4.0 * m) ** 2)


def _flat(o, d, L, tmin, tmax, S, m, n, k, inside):
    """pairs of a ray (o, d, L = |d|, tmin, tmax) and a plane n.x = k; inside(x_dot) -> signed distance of the crossing from the shape's boundary, positive
    inside, given a function x_dot(w) -> w . crossing.  -> t (ray parameter), hit, close"""
    den = (d * n).sum(1) / L                                            # cos of the ray with the normal
    h = k - (o * n).sum(1)                                              # signed distance of the origin from the plane
    par = den == 0
    tu = np.where(par, 0.0, h / np.where(par, 1.0, den))                # distance along the ray (parallel rays: masked out below)
    t = tu / L

    def x_dot(w):
        return (o * w).sum(1) + t * (d * w).sum(1)
    e = inside(x_dot)
    T0, T1 = tmin * L, tmax * L
    mt = m * np.maximum(1.0, np.abs(tu) / S)
    c = np.abs(den)
    g = np.where(c < GRAZING, m / np.where(par, 1.0, c), 0.0)            # how far either side of the crossing a grazing ray stays within m of the plane
    hit = ~par & (e > 0) & (t > tmin) & (t < tmax)
    near = ~par & (e > -(m + g)) & (tu > T0 - mt - g) & (tu < T1 + mt + g)
    clear = (c >= GRAZING) & (e >= m) & (tu >= T0 + mt) & (tu <= T1 - mt)
    close = near & ~clear
    close |= par & (np.abs(h) <= m)                                      # parallel to the plane, within m of it, its line near the shape (_pairs)
    return t, hit, close


def cast(sh, o, d, tmin, tmax):
    """rays (o, d) (n, 3), tmin, tmax (n,) -> dict(prim: nearest primitive hit inside (tmin, tmax) or -1, t: its ray parameter (inf on a miss), t2: the
    runner-up's (inf if none), hit, decisive: the verdict `hit` is beyond doubt, unique: so are the primitive and t -- no close call at all, and the runner-up
    is farther by more than 4 m')"""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    tmin = np.asarray(tmin, np.float64); tmax = np.asarray(tmax, np.float64)
    N = o.shape[0]
    S, m = sh.S, sh.m
    best = _Best(N)
    L = np.linalg.norm(d, axis=1)
    du = d / L[:, None]
    biggest = max(len(sh.tri_prim), len(sh.rect_prim), len(sh.sph_prim), len(sh.disk_prim), 1)
    step = max(256, min(N, (1 << 22) // biggest))
    for a in range(0, N, step):
        sl = slice(a, min(N, a + step))
        for P in sh._polys:
            if P is None:
                continue
            ri, pi = _pairs(o[sl], du[sl], P["centre"], P["radius"], m)
            ri += a

            def inside(x_dot, P=P, pi=pi):
                e = None
                for w, kw in zip(P["W"], P["KW"]):
                    ei = x_dot(w[pi]) - kw[pi]
                    e = ei if e is None else np.minimum(e, ei)
                return e
            best.add(ri, *_flat(o[ri], d[ri], L[ri], tmin[ri], tmax[ri], S, m, P["n"][pi], P["k"][pi], inside), P["prim"][pi])
        if len(sh.disk_prim):
            n, c, r = sh.disk_n, sh.disk_c, sh.disk_r
            ri, pi = _pairs(o[sl], du[sl], c, r, m)
            ri += a

            def inside(x_dot, pi=pi):
                # |crossing - centre| from the three coordinates of the crossing
                x = [x_dot(np.broadcast_to(ax, (len(pi), 3))) - c[pi, i] for i, ax in enumerate(np.eye(3))]
                return r[pi] - np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
            best.add(ri, *_flat(o[ri], d[ri], L[ri], tmin[ri], tmax[ri], S, m, n[pi], (c * n).sum(1)[pi], inside), sh.disk_prim[pi])
        if len(sh.sph_prim):
            ri, pi = _pairs(o[sl], du[sl], sh.sph_c, sh.sph_r, m)
            ri += a
            c, r = sh.sph_c[pi], sh.sph_r[pi]
            oc = o[ri] - c
            b = (oc * du[ri]).sum(1)
            disc = b * b - ((oc * oc).sum(1) - r * r)
            sq = np.sqrt(np.maximum(disc, 0.0))
            ra, rb = -b - sq, -b + sq                                   # distances along the ray
            T0, T1 = tmin[ri] * L[ri], tmax[ri] * L[ri]
            in_a = (disc > 0) & (ra > T0) & (ra < T1); in_b = (disc > 0) & (rb > T0) & (rb < T1)
            tu = np.where(in_a, ra, rb)
            tang = np.abs(disc) <= m * (2.0 * r + m)
            ma, mb = m * np.maximum(1.0, np.abs(ra) / S), m * np.maximum(1.0, np.abs(rb) / S)
            edge = (disc > 0) & ((np.abs(ra - T0) <= ma) | (np.abs(ra - T1) <= ma) | (np.abs(rb - T0) <= mb) | (np.abs(rb - T1) <= mb))
            mc = m * np.maximum(1.0, np.abs(b) / S) + 2.0 * np.sqrt(m * r)   # a tangent ray touches at -b, give or take sqrt(2 r m)
            close = edge | (tang & (-b > T0 - mc) & (-b < T1 + mc))
            best.add(ri, tu / L[ri], in_a | in_b, close, sh.sph_prim[pi])
    hit = best.prim >= 0
    mp = m * np.maximum(1.0, np.where(hit, best.t1, 0.0) / S)
    unique = hit & (np.where(hit, best.t2, np.inf) - np.where(hit, best.t1, 0.0) > 4.0 * mp)
    return dict(prim=best.prim, t=best.t1, t2=best.t2, hit=hit, decisive=~best.close | best.blocked, unique=unique & ~best.close)
