"""Plain-numpy decoders of the hierarchy tables an upload puts on the device, and a validator that says "this is a valid tree over these primitives".

Written from the format comments of csrc/jp_device.h and the builders (csrc/jp_scene_host.h, jp_lbvh.h, jp_ploc.h); imports nothing from the library.  TEST
INFRASTRUCTURE.  Every statement checked is exact (tables are integers and fp32 values; fp32 arithmetic is restated with numpy float32, whose + - * / are the
same single correctly rounded IEEE operations the builders run).  The walks go level by level with numpy frontiers: no Python loop per node.

    tabs:  {"nodes" | "prims" | "meta" | "wide" | "q4" | "flat": uint8 array}     (an absent or empty entry: the upload has no such table)
    info:  {"n_prims", "n_nodes", "bvh_height", "n_wide", "wide_height", "n_q4", "q4_height"}
    validate(tabs, info, ...) -> Report; Report.errors is a list of (kind, message), kind one of
        "bounds" "partition" "permutation" "leaf_size" "containment" "tightness" "height" "cover" "order" "topology"
"""
import bisect

import numpy as np

F = np.float32
TRIANGLE, RECTANGLE, SPHERE, DISK = 0, 1, 2, 3
EMPTY = np.zeros(0, np.uint8)


class Report:
    def __init__(self):
        self.errors = []
        self.stats = {}

    def add(self, kind, msg):
        self.errors.append((kind, msg))

    def where(self, bad, kind, fmt):
        """bad: boolean array; reports the first offender through fmt(index tuple)"""
        bad = np.asarray(bad)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            self.add(kind, "%s (%d in all)" % (fmt(i), int(bad.sum())))
            return True
        return False

    def kinds(self):
        return {k for k, _ in self.errors}

    def ok(self):
        return not self.errors

    def __str__(self):
        return "\n".join("%s: %s" % e for e in self.errors) or "valid"


# ---- decoders ---------------------------------------------------------------------------------------------------------------------
def _words(b, per, dtype):
    b = np.ascontiguousarray(b if b is not None else EMPTY, np.uint8)
    assert b.size % (4 * per) == 0, "table is no whole number of %d-word records" % per
    return b.view(dtype).reshape(-1, per)


def decode_prims(b):
    """primitive records: four float4 (jp_scene_host.h emit_prim) -> (n, 16) float32; the shape type is the int in word 15"""
    return _words(b, 16, np.float32)


def decode_meta(b):
    """(caller's primitive index, material, light, shape type) -> (n, 4) int32"""
    return _words(b, 4, np.int32)


def decode_binary(b):
    """binary node: four float4 = left box (lo xyz, hi xyz), right box, left ref, right ref, two zeros
    -> box (n, 2, 6) float32, refs (n, 2) int32, raw (n, 16) uint32.  ref >= 0: node; ref < 0: leaf -(((first << 4) | (count - 1)) + 1)"""
    raw = _words(b, 16, np.uint32)
    return raw[:, :12].copy().view(np.float32).reshape(-1, 2, 6), raw[:, 12:14].copy().view(np.int32), raw


def leaf_range(ref):
    e = -np.asarray(ref, np.int64) - 1
    return e >> 4, (e & 15) + 1


def leaf_ref(first, count):
    return -(((np.asarray(first, np.int64) << 4) | (np.asarray(count, np.int64) - 1)) + 1)


def _exps(w3):
    return np.stack([(w3 >> (8 * a)) & 255 for a in range(3)], axis=1).astype(np.int64) - 127


def decode_wide8(b):
    """8-wide node, twenty words: origin xyz, (ex | ey << 8 | ez << 16 | imask << 24), child_base, prim_base, eight meta bytes, 6 x 8 plane bytes
    (lo x, lo y, lo z, hi x, hi y, hi z; byte k of a group = slot k).  meta: 0 empty; inner 0x20 | (24 + slot); chunk (unary count << 5) | offset"""
    w = _words(b, 20, np.uint32)
    return dict(origin=w[:, :3].copy().view(np.float32), exp=_exps(w[:, 3]), imask=(w[:, 3] >> 24).astype(np.int64), child_base=w[:, 4].astype(np.int64),
                prim_base=w[:, 5].astype(np.int64), meta=w[:, 6:8].copy().view(np.uint8).reshape(-1, 8).astype(np.int64),
                planes=w[:, 8:20].copy().view(np.uint8).reshape(-1, 6, 8).astype(np.int64), raw=w)


def decode_q4(b):
    """4-wide node, sixteen words: origin xyz, (ex | ey << 8 | ez << 16 | valid << 24), four refs (node index, or a leaf ref as in the binary tree),
    6 x 4 plane bytes (lo x, lo y, lo z, hi x, hi y, hi z), flags, 0"""
    w = _words(b, 16, np.uint32)
    return dict(origin=w[:, :3].copy().view(np.float32), exp=_exps(w[:, 3]), valid=(w[:, 3] >> 24).astype(np.int64), refs=w[:, 4:8].copy().view(np.int32).astype(np.int64),
                planes=w[:, 8:14].copy().view(np.uint8).reshape(-1, 6, 4).astype(np.int64), flags=w[:, 14], raw=w)


def decode_flat(b):
    """flat leaf list, two float4 per leaf: (lo xyz, low mask word) (hi xyz, high mask word) -> box (n, 6) float32, bits (n,) uint64"""
    w = _words(b, 8, np.uint32)
    f = w.view(np.float32)
    return np.concatenate([f[:, 0:3], f[:, 4:7]], axis=1), w[:, 3].astype(np.uint64) | (w[:, 7].astype(np.uint64) << np.uint64(32))


def dequantise(origin, exp, planes):
    """plane = fmaf(q, 2^e, origin) as the walks evaluate it: one rounding of the exact value -> (n, 6, slots) float32"""
    sc = np.ldexp(1.0, exp)                                             # (n, 3) float64, exact
    o = origin.astype(np.float64)
    sc6 = np.concatenate([sc, sc], axis=1)[:, :, None]; o6 = np.concatenate([o, o], axis=1)[:, :, None]
    return (planes.astype(np.float64) * sc6 + o6).astype(np.float32)    # q * 2^e is exact in float64; the sum has 53 bits, so this is fmaf unless the exponents lie > 29 bits apart


# ---- primitive extents ------------------------------------------------------------------------------------------------------------
def prim_types(prims):
    return prims[:, 15].copy().view(np.int32)


def prim_extents(prims, disk="sphere"):
    """exact extents per record, as k_lbvh_bounds computes them in fp32 (all operations here are float32): sphere and disk centre -+ radius, triangle min / max of
    the vertices, rectangle also the fourth corner carried in the .w components.  disk="tight": the disk's own extent r * sqrt(1 - n_a^2) per axis, in
    double -- what a host-built tree has to contain (its caller boxes a disk by the square spanned in its plane, not by its bounding sphere)"""
    t = prim_types(prims)
    g0, g1, g2 = prims[:, 0:3], prims[:, 4:7], prims[:, 8:11]
    lo = np.minimum(np.minimum(g0, g1), g2); hi = np.maximum(np.maximum(g0, g1), g2)
    g3 = np.stack([prims[:, 3], prims[:, 7], prims[:, 11]], axis=1)
    r = t == RECTANGLE
    lo = np.where(r[:, None], np.minimum(lo, g3), lo); hi = np.where(r[:, None], np.maximum(hi, g3), hi)
    s = (t == SPHERE) | (t == DISK)
    rad = prims[:, 3:4]
    lo = np.where(s[:, None], g0 - rad, lo); hi = np.where(s[:, None], g0 + rad, hi)
    lo = lo.astype(np.float64); hi = hi.astype(np.float64)
    if disk == "tight":
        d = t == DISK
        n = g1.astype(np.float64); nn = np.maximum((n * n).sum(1, keepdims=True), 1e-300)
        ext = rad.astype(np.float64) * np.sqrt(np.maximum(0.0, 1.0 - n * n / nn))
        lo = np.where(d[:, None], g0 - ext, lo); hi = np.where(d[:, None], g0 + ext, hi)
    return lo, hi


def lbvh_pad(lo, hi):
    """the relative pad of every child box (jp_lbvh.h lbvh_pad, jp_scene_host.h padded_box): fp32, operation by operation"""
    lo = lo.astype(F); hi = hi.astype(F)
    e = np.maximum(np.abs(lo), np.abs(hi)) * F(1e-6) + F(1e-6)
    return lo - e, hi + e


def _range_union(first, count, elo, ehi, n):
    """union of the extents of positions first .. first + count - 1, count <= 24: one vectorised pass per position in the range"""
    lo = np.full((first.size, 3), np.inf); hi = np.full((first.size, 3), -np.inf)
    if first.size == 0 or n == 0:
        return lo, hi
    for j in range(int(min(count.max(), 24))):
        idx = np.clip(first + np.minimum(j, count - 1), 0, n - 1)
        lo = np.minimum(lo, elo[idx]); hi = np.maximum(hi, ehi[idx])
    return lo, hi


def _coverage(first, count, n):
    d = np.zeros(n + 1, np.int64)
    ok = (first >= 0) & (count >= 1) & (first + count <= n)
    np.add.at(d, first[ok], 1); np.add.at(d, (first + count)[ok], -1)
    return np.cumsum(d)[:n]


def _key(minfirst, count):
    return (np.asarray(minfirst, np.int64) << 32) | np.asarray(count, np.int64)


# ---- the binary tree --------------------------------------------------------------------------------------------------------------
def walk_binary(rep, nodes_b, n_prims, n_nodes_reported, elo, ehi, max_leaf=16, dense=False, tight=False):
    """partition, leaf sizes, containment, (device builds) tightness; -> what the wide trees are compared with"""
    box, refs, raw = decode_binary(nodes_b)
    n_nodes = refs.shape[0]
    if n_nodes != n_nodes_reported:
        rep.add("bounds", "binary table holds %d nodes, %d reported" % (n_nodes, n_nodes_reported))
    out = dict(height=0, leaf_first=np.zeros(0, np.int64), leaf_count=np.zeros(0, np.int64), keys=np.zeros(0, np.int64), key_box=np.zeros((0, 6), F))
    if n_nodes == 0:
        rep.add("bounds", "no binary nodes"); return out
    seen = np.zeros(n_nodes, bool)
    void = (box[:, :, :3] > box[:, :, 3:]).any(2)                      # the empty box beside the only leaf of a one-leaf tree: no ray enters it, its reference repeats the leaf's
    levels, lf_node, lf_side = [], [], []
    frontier = np.array([0], np.int64)
    while frontier.size:
        oob = (frontier < 0) | (frontier >= n_nodes)
        rep.where(oob, "bounds", lambda i: "binary child reference %d past n_nodes %d at depth %d" % (frontier[i[0]], n_nodes, len(levels)))
        frontier = frontier[~oob]
        uniq, cnt = np.unique(frontier, return_counts=True)
        again = (cnt > 1) | seen[uniq]
        rep.where(again, "partition", lambda i: "binary node %d is reached more than once" % uniq[i[0]])
        frontier = uniq[~seen[uniq]]
        if not frontier.size:
            break
        seen[frontier] = True; levels.append(frontier)
        r = refs[frontier]
        for s in range(2):
            m = (r[:, s] < 0) & ~void[frontier, s]
            lf_node.append(frontier[m]); lf_side.append(np.full(int(m.sum()), s, np.int64))
        frontier = r[r >= 0].astype(np.int64)
    out["height"] = len(levels)
    lf_node = np.concatenate(lf_node); lf_side = np.concatenate(lf_side)
    first, count = leaf_range(refs[lf_node, lf_side])
    rep.where((first < 0) | (first + count > n_prims), "bounds", lambda i: "binary leaf of node %d covers %d .. %d, n_prims %d" % (lf_node[i[0]], first[i[0]], first[i[0]] + count[i[0]] - 1, n_prims))
    rep.where(count > max_leaf, "leaf_size", lambda i: "binary leaf of node %d holds %d primitives, limit %d" % (lf_node[i[0]], count[i[0]], max_leaf))
    cov = _coverage(first, count, n_prims)
    rep.where(cov != 1, "partition", lambda i: "primitive position %d is in %d binary leaves" % (i[0], cov[i[0]]))
    if dense:
        rep.where(~seen, "partition", lambda i: "binary node %d is never reached" % i[0])
    else:
        rep.where(~seen & (raw != 0).any(1), "partition", lambda i: "binary node %d is not reached and not all-zero" % i[0])
    # bottom-up: the exact union, the smallest position and the primitive count below every child
    cu_lo = np.full((n_nodes, 2, 3), np.inf); cu_hi = np.full((n_nodes, 2, 3), -np.inf)
    cmin = np.full((n_nodes, 2), np.iinfo(np.int64).max, np.int64); ccnt = np.zeros((n_nodes, 2), np.int64)
    ulo, uhi = _range_union(first, count, elo, ehi, n_prims)
    cu_lo[lf_node, lf_side] = ulo; cu_hi[lf_node, lf_side] = uhi; cmin[lf_node, lf_side] = first; ccnt[lf_node, lf_side] = count
    for lv in reversed(levels):
        r = refs[lv]
        for s in range(2):
            m = (r[:, s] >= 0) & (r[:, s] < n_nodes)
            c = r[m, s]
            cu_lo[lv[m], s] = cu_lo[c].min(1); cu_hi[lv[m], s] = cu_hi[c].max(1); cmin[lv[m], s] = cmin[c].min(1); ccnt[lv[m], s] = ccnt[c].sum(1)
    live = np.concatenate(levels)
    b = box[live].astype(np.float64)
    with np.errstate(invalid="ignore"):
        rep.where((b[:, :, :3] > cu_lo[live]) | (b[:, :, 3:] < cu_hi[live]), "containment",
                  lambda i: "binary node %d child %d axis %d: box [%.9g, %.9g] does not contain the primitives below it [%.9g, %.9g]"
                  % (live[i[0]], i[1], i[2], b[i[0], i[1], i[2]], b[i[0], i[1], 3 + i[2]], cu_lo[live[i[0]], i[1], i[2]], cu_hi[live[i[0]], i[1], i[2]]))
        if tight:
            # one-sided: not looser than the lbvh_pad image of the exact union, computed in fp32 and widened by one ulp (m * 1e-6f + 1e-6f may be contracted)
            fin = np.isfinite(cu_lo[live]).all(2) & np.isfinite(cu_hi[live]).all(2)
            plo, phi = lbvh_pad(np.where(fin[:, :, None], cu_lo[live], 0.0), np.where(fin[:, :, None], cu_hi[live], 0.0))
            bf = box[live]
            wlo = np.nextafter(plo, F(-np.inf)); whi = np.nextafter(phi, F(np.inf))
            rep.where(fin[:, :, None] & ((bf[:, :, :3] < wlo) | (bf[:, :, 3:] > whi)), "tightness",
                      lambda i: "binary node %d child %d axis %d: box [%.9g, %.9g] is looser than the padded union [%.9g, %.9g]"
                      % (live[i[0]], i[1], i[2], bf[i[0], i[1], i[2]], bf[i[0], i[1], 3 + i[2]], wlo[i], whi[i]))
            # ... and no tighter: min and max are exact, so the builders' unions are THE unions, and a padded box that is more than that one ulp inside the
            # image was padded from a box that missed a primitive by less than the pad (a stale child box in the refit), which containment alone lets pass
            nlo = np.nextafter(plo, F(np.inf)); nhi = np.nextafter(phi, F(-np.inf))
            rep.where(fin[:, :, None] & ((bf[:, :, :3] > nlo) | (bf[:, :, 3:] < nhi)), "tightness",
                      lambda i: "binary node %d child %d axis %d: box [%.9g, %.9g] is tighter than the padded union [%.9g, %.9g]"
                      % (live[i[0]], i[1], i[2], bf[i[0], i[1], i[2]], bf[i[0], i[1], 3 + i[2]], nlo[i], nhi[i]))
    real = (ccnt[live] > 0)                                             # (the synthetic root of a one-leaf tree repeats its leaf: keep one)
    keys = _key(cmin[live][real], ccnt[live][real]); kb = box[live][real]
    o = np.argsort(keys, kind="stable")
    out.update(leaf_first=first, leaf_count=count, keys=keys[o], key_box=kb[o], refs=refs, box=box, levels=levels, seen=seen)
    return out


def _lookup(binary, minfirst, count):
    """the binary tree's child box over exactly these primitives (smallest position, count) -> found mask, boxes"""
    k = _key(minfirst, count)
    keys = binary["keys"]
    if keys.size == 0:
        return np.zeros(k.shape, bool), np.zeros(k.shape + (6,), F)
    at = np.clip(np.searchsorted(keys, k), 0, keys.size - 1)
    return keys[at] == k, binary["key_box"][at]


def _check_scale(rep, name, lo, hi, exp, nodes):
    """e is the smallest exponent (from ceil(log2(extent / 255)), at least -120) for which 255 steps span the node's extent, or that plus one: log2f is approximate
    and the builders only correct upward"""
    lo = lo.astype(F); hi = hi.astype(F)
    x = np.maximum((hi - lo) / F(255.0), F(1e-30)).astype(np.float64)
    e0 = np.clip(np.ceil(np.log2(x)), -120, 120).astype(np.int64)
    spans = lambda e: (255.0 * np.ldexp(1.0, e) + lo.astype(np.float64)).astype(F) >= hi
    need = np.where(spans(e0), e0, np.where(spans(e0 + 1), e0 + 1, e0 + 2))
    rep.where((exp < need) | (exp > need + 1), "tightness", lambda i: "%s node %d axis %d: scale exponent %d, expected %d or %d for the extent [%.9g, %.9g]"
              % (name, nodes[i[0]], i[1], exp[i], need[i], need[i] + 1, lo[i], hi[i]))


def _check_planes(rep, name, nodes, present, deq, qbox, exp, extent_lo, extent_hi):
    """a quantised plane encloses the box it quantises and lies within one step 2^e of it.  The builders take floor / ceil of fl(b - lo) / 2^e: the subtraction's
    rounding (relative 2^-24) can cost a further step's hair, and the plane itself is rounded once: both are allowed for, nothing else"""
    step = np.ldexp(1.0, exp)[:, :, None]                               # (k, 3, 1)
    d = deq.astype(np.float64); q = qbox.astype(np.float64)             # (k, 6, slots)
    span = np.maximum(np.abs(extent_hi.astype(np.float64) - extent_lo.astype(np.float64)), 0.0)[:, :, None]
    mag = np.maximum(np.abs(extent_lo), np.abs(extent_hi)).astype(np.float64)[:, :, None]
    slack = span * 2.0 ** -23 + mag * 2.0 ** -23
    p = present[:, None, :]
    rep.where(p & ((d[:, :3] > q[:, :3]) | (d[:, 3:] < q[:, 3:])), "containment",
              lambda i: "%s node %d axis %d slot %d: planes [%.9g, %.9g] do not enclose the box they quantise [%.9g, %.9g]" % (name, nodes[i[0]], i[1], i[2], d[i[0], i[1], i[2]], d[i[0], 3 + i[1], i[2]], q[i[0], i[1], i[2]], q[i[0], 3 + i[1], i[2]]))
    rep.where(p & ((d[:, :3] < q[:, :3] - step - slack) | (d[:, 3:] > q[:, 3:] + step + slack)), "tightness",
              lambda i: "%s node %d axis %d slot %d: planes [%.9g, %.9g] lie more than one step %.3g from the box they quantise [%.9g, %.9g]"
              % (name, nodes[i[0]], i[1], i[2], d[i[0], i[1], i[2]], d[i[0], 3 + i[1], i[2]], step[i[0], i[1], 0], q[i[0], i[1], i[2]], q[i[0], 3 + i[1], i[2]]))


def _walk_wide_levels(rep, name, n, children_of):
    """frontier walk shared by the two wide formats -> levels, seen"""
    seen = np.zeros(n, bool); levels = []
    frontier = np.array([0], np.int64)
    while frontier.size:
        oob = (frontier < 0) | (frontier >= n)
        rep.where(oob, "bounds", lambda i: "%s child index %d past the %d nodes" % (name, frontier[i[0]], n))
        frontier = frontier[~oob]
        uniq, cnt = np.unique(frontier, return_counts=True)
        rep.where((cnt > 1) | seen[uniq], "partition", lambda i: "%s node %d is reached more than once" % (name, uniq[i[0]]))
        frontier = uniq[~seen[uniq]]
        if not frontier.size:
            break
        seen[frontier] = True; levels.append(frontier)
        frontier = children_of(frontier)
    rep.where(~seen, "partition", lambda i: "%s node %d is never reached (the nodes reached must number exactly the nodes reported)" % (name, i[0]))
    return levels, seen


# ---- the 4-wide tree --------------------------------------------------------------------------------------------------------------
def walk_q4(rep, q4_b, n_prims, n_q4_reported, elo, ehi, binary, max_leaf=16):
    q = decode_q4(q4_b)
    n = q["refs"].shape[0]
    if n != n_q4_reported:
        rep.add("bounds", "4-wide table holds %d nodes, %d reported" % (n, n_q4_reported))
    if n == 0:
        return 0
    slot = np.arange(4)
    valid = ((q["valid"][:, None] >> slot) & 1).astype(bool)
    refs = q["refs"]
    inner = valid & (refs >= 0); leaf = valid & (refs < 0)
    levels, seen = _walk_wide_levels(rep, "4-wide", n, lambda f: refs[f][inner[f]])
    live = np.concatenate(levels)
    rep.where(valid[live].sum(1) < 2, "topology", lambda i: "4-wide node %d has fewer than two children" % live[i[0]])
    ln, ls = np.nonzero(leaf & seen[:, None])
    first, count = leaf_range(refs[ln, ls])
    rep.where((first < 0) | (first + count > n_prims), "bounds", lambda i: "4-wide leaf of node %d covers %d .. %d, n_prims %d" % (ln[i[0]], first[i[0]], first[i[0]] + count[i[0]] - 1, n_prims))
    rep.where(count > max_leaf, "leaf_size", lambda i: "4-wide leaf of node %d holds %d primitives, limit %d" % (ln[i[0]], count[i[0]], max_leaf))
    cov = _coverage(first, count, n_prims)
    rep.where(cov != 1, "partition", lambda i: "primitive position %d is in %d 4-wide leaves" % (i[0], cov[i[0]]))
    # the same leaves as the binary tree
    a = np.sort(_key(first, count)); b = np.sort(_key(binary["leaf_first"], binary["leaf_count"]))
    if a.size != b.size or (a != b).any():
        rep.add("cover", "the 4-wide tree's leaf references are not the binary tree's (%d against %d leaves)" % (a.size, b.size))
    # bottom-up
    cu_lo = np.full((n, 4, 3), np.inf); cu_hi = np.full((n, 4, 3), -np.inf); cmin = np.full((n, 4), np.iinfo(np.int64).max, np.int64); ccnt = np.zeros((n, 4), np.int64)
    ulo, uhi = _range_union(first, count, elo, ehi, n_prims)
    cu_lo[ln, ls] = ulo; cu_hi[ln, ls] = uhi; cmin[ln, ls] = first; ccnt[ln, ls] = count
    for lv in reversed(levels):
        for s in range(4):
            m = inner[lv, s] & (refs[lv, s] < n)
            c = refs[lv[m], s]
            cu_lo[lv[m], s] = cu_lo[c].min(1); cu_hi[lv[m], s] = cu_hi[c].max(1); cmin[lv[m], s] = cmin[c].min(1); ccnt[lv[m], s] = ccnt[c].sum(1)
    deq = dequantise(q["origin"][live], q["exp"][live], q["planes"][live])           # (k, 6, 4)
    d = deq.astype(np.float64); v = valid[live]
    lo_u = np.transpose(cu_lo[live], (0, 2, 1)); hi_u = np.transpose(cu_hi[live], (0, 2, 1))   # (k, 3, 4)
    rep.where(v[:, None, :] & ((d[:, :3] > lo_u) | (d[:, 3:] < hi_u)), "containment",
              lambda i: "4-wide node %d axis %d slot %d: planes [%.9g, %.9g] do not contain the primitives below [%.9g, %.9g]" % (live[i[0]], i[1], i[2], d[i[0], i[1], i[2]], d[i[0], 3 + i[1], i[2]], lo_u[i], hi_u[i]))
    # against the binary child box each slot quantises: box -+ 1e-6 of the node's extent, the node's own box widened likewise
    found, bb = _lookup(binary, cmin[live], ccnt[live])                            # (k, 4), (k, 4, 6)
    rep.where(v & ~found, "cover", lambda i: "4-wide node %d slot %d covers %d primitives from position %d: the binary tree has no such child" % (live[i[0]], i[1], ccnt[live[i[0]], i[1]], cmin[live[i[0]], i[1]]))
    ok = v & found
    nlo = np.where(ok[:, :, None], bb[:, :, :3], F(np.inf)).min(1); nhi = np.where(ok[:, :, None], bb[:, :, 3:], F(-np.inf)).max(1)   # (k, 3) float32
    some = ok.any(1)
    nlo = np.where(some[:, None], nlo, F(0)); nhi = np.where(some[:, None], nhi, F(0))
    ex = F(1e-6) * (nhi - nlo)
    plo = nlo - ex; phi = nhi + ex
    qlo = np.transpose(bb[:, :, :3], (0, 2, 1)) - ex[:, :, None]; qhi = np.transpose(bb[:, :, 3:], (0, 2, 1)) + ex[:, :, None]
    full = ok.sum(1) == v.sum(1)
    org = q["origin"][live]
    rep.where(full[:, None] & (np.abs(org.astype(np.float64) - plo) > np.spacing(np.abs(plo)).astype(np.float64)), "tightness",
              lambda i: "4-wide node %d axis %d: origin %.9g, the children's boxes start at %.9g" % (live[i[0]], i[1], org[i], plo[i]))
    _check_scale(rep, "4-wide", np.where(full[:, None], org, F(0)), np.where(full[:, None], phi, F(0)), np.where(full[:, None], q["exp"][live], -99), live)
    _check_planes(rep, "4-wide", live, ok, deq, np.concatenate([qlo, qhi], axis=1), q["exp"][live], plo, phi)
    return len(levels)


# ---- the 8-wide tree --------------------------------------------------------------------------------------------------------------
def walk_wide8(rep, wide_b, n_prims, n_wide_reported, elo, ehi, binary):
    w = decode_wide8(wide_b)
    n = w["meta"].shape[0]
    if n != n_wide_reported:
        rep.add("bounds", "8-wide table holds %d nodes, %d reported" % (n, n_wide_reported))
    if n == 0:
        return 0
    meta = w["meta"]; slot = np.arange(8)
    inner = (meta != 0) & ((meta & 0x18) == 0x18)
    chunk = (meta != 0) & ~inner
    rank = np.cumsum(inner, axis=1) - inner                            # inner children are contiguous from child_base, in slot order
    child = w["child_base"][:, None] + rank
    levels, seen = _walk_wide_levels(rep, "8-wide", n, lambda f: child[f][inner[f]])
    live = np.concatenate(levels)
    im = ((w["imask"][:, None] >> slot) & 1).astype(bool)
    rep.where(seen[:, None] & (im != inner), "topology", lambda i: "8-wide node %d slot %d: inner mask and meta byte %#x disagree" % (i[0], i[1], meta[i]))
    rep.where(seen[:, None] & inner & ((meta & 7) != slot), "topology", lambda i: "8-wide node %d slot %d: inner meta byte %#x names another slot" % (i[0], i[1], meta[i]))
    cn, cs = np.nonzero(chunk & seen[:, None])
    bits = meta[cn, cs] >> 5; off = meta[cn, cs] & 31
    count = np.where(bits == 1, 1, np.where(bits == 3, 2, np.where(bits == 7, 3, -1)))
    rep.where(count < 0, "leaf_size", lambda i: "8-wide node %d slot %d: chunk bits %#x are no unary count of 1 .. 3" % (cn[i[0]], cs[i[0]], bits[i[0]]))
    count = np.where(count < 0, 1, count)
    rep.where(off + count > 24, "leaf_size", lambda i: "8-wide node %d slot %d: chunk at offset %d + %d leaves the 24-record window" % (cn[i[0]], cs[i[0]], off[i[0]], count[i[0]]))
    first = w["prim_base"][cn] + off
    rep.where((first < 0) | (first + count > n_prims), "bounds", lambda i: "8-wide chunk of node %d covers %d .. %d, n_prims %d" % (cn[i[0]], first[i[0]], first[i[0]] + count[i[0]] - 1, n_prims))
    cov = _coverage(first, count, n_prims)
    rep.where(cov != 1, "partition", lambda i: "primitive position %d is in %d 8-wide leaf chunks" % (i[0], cov[i[0]]))
    # every chunk lies inside one leaf of the binary tree (with the partition above: the chunks tile the binary tree's leaves)
    lf = binary["leaf_first"]; lc = binary["leaf_count"]
    o = np.argsort(lf, kind="stable"); lf = lf[o]; lc = lc[o]
    cbox = np.zeros((first.size, 6), F); inleaf = np.zeros(first.size, bool)
    if lf.size:
        at = np.clip(np.searchsorted(lf, first, side="right") - 1, 0, lf.size - 1)
        inleaf = (lf[at] <= first) & (first + count <= lf[at] + lc[at])
        found, cbox = _lookup(binary, lf[at], lc[at]); inleaf &= found
    rep.where(~inleaf, "cover", lambda i: "8-wide chunk %d .. %d of node %d lies in no single leaf of the binary tree" % (first[i[0]], first[i[0]] + count[i[0]] - 1, cn[i[0]]))
    # bottom-up
    cu_lo = np.full((n, 8, 3), np.inf); cu_hi = np.full((n, 8, 3), -np.inf); cmin = np.full((n, 8), np.iinfo(np.int64).max, np.int64); ccnt = np.zeros((n, 8), np.int64)
    ulo, uhi = _range_union(first, count, elo, ehi, n_prims)
    cu_lo[cn, cs] = ulo; cu_hi[cn, cs] = uhi; cmin[cn, cs] = first; ccnt[cn, cs] = count
    for lv in reversed(levels):
        for s in range(8):
            m = inner[lv, s] & (child[lv, s] < n)
            c = child[lv[m], s]
            cu_lo[lv[m], s] = cu_lo[c].min(1); cu_hi[lv[m], s] = cu_hi[c].max(1); cmin[lv[m], s] = cmin[c].min(1); ccnt[lv[m], s] = ccnt[c].sum(1)
    present = (inner | chunk)[live]
    deq = dequantise(w["origin"][live], w["exp"][live], w["planes"][live])         # (k, 6, 8)
    d = deq.astype(np.float64)
    lo_u = np.transpose(cu_lo[live], (0, 2, 1)); hi_u = np.transpose(cu_hi[live], (0, 2, 1))
    rep.where(present[:, None, :] & ((d[:, :3] > lo_u) | (d[:, 3:] < hi_u)), "containment",
              lambda i: "8-wide node %d axis %d slot %d: planes [%.9g, %.9g] do not contain the primitives below [%.9g, %.9g]" % (live[i[0]], i[1], i[2], d[i[0], i[1], i[2]], d[i[0], 3 + i[1], i[2]], lo_u[i], hi_u[i]))
    # the binary child box each slot quantises: an inner slot the child over the same primitives, a chunk slot its leaf
    found, bb = _lookup(binary, cmin[live], ccnt[live])                            # (k, 8), (k, 8, 6)
    rep.where(inner[live] & ~found, "cover", lambda i: "8-wide node %d slot %d covers %d primitives from position %d: the binary tree has no such child" % (live[i[0]], i[1], ccnt[live[i[0]], i[1]], cmin[live[i[0]], i[1]]))
    qb = np.zeros((n, 8, 6), F); have = np.zeros((n, 8), bool)
    qb[live] = np.where((inner[live] & found)[:, :, None], bb, F(0)); have[live] = inner[live] & found
    qb[cn, cs] = np.where(inleaf[:, None], cbox, F(0)); have[cn, cs] = inleaf
    qb = qb[live]; ok = have[live]
    nlo = np.where(ok[:, :, None], qb[:, :, :3], F(np.inf)).min(1); nhi = np.where(ok[:, :, None], qb[:, :, 3:], F(-np.inf)).max(1)
    some = ok.any(1); nlo = np.where(some[:, None], nlo, F(0)); nhi = np.where(some[:, None], nhi, F(0))
    full = ok.sum(1) == present.sum(1)
    org = w["origin"][live]
    rep.where(full[:, None] & (org != nlo), "tightness", lambda i: "8-wide node %d axis %d: origin %.9g, the children's boxes start at %.9g" % (live[i[0]], i[1], org[i], nlo[i]))
    _check_scale(rep, "8-wide", np.where(full[:, None], org, F(0)), np.where(full[:, None], nhi, F(0)), np.where(full[:, None], w["exp"][live], -99), live)
    _check_planes(rep, "8-wide", live, ok, deq, np.transpose(qb, (0, 2, 1)), w["exp"][live], nlo, nhi)
    return len(levels)


# ---- the flat leaf list -----------------------------------------------------------------------------------------------------------
def check_flat(rep, flat_b, n_prims, elo, ehi, binary):
    box, bits = decode_flat(flat_b)
    if box.shape[0] == 0:
        return
    if n_prims > 64:
        rep.add("bounds", "a flat leaf list over %d primitives: the masks hold 64" % n_prims); return
    member = ((bits[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)   # (leaves, 64)
    rep.where(member[:, n_prims:].any(1), "bounds", lambda i: "flat leaf %d names a primitive past n_prims %d" % (i[0], n_prims))
    cov = member[:, :n_prims].sum(0)
    rep.where(cov != 1, "partition", lambda i: "primitive position %d is in %d flat leaves" % (i[0], cov[i[0]]))
    m = member[:, :n_prims]
    lo = np.where(m[:, :, None], elo[None, :n_prims], np.inf).min(1); hi = np.where(m[:, :, None], ehi[None, :n_prims], -np.inf).max(1)
    b = box.astype(np.float64)
    rep.where((b[:, :3] > lo) | (b[:, 3:] < hi), "containment", lambda i: "flat leaf %d axis %d: box [%.9g, %.9g] does not contain its primitives [%.9g, %.9g]" % (i[0], i[1], b[i[0], i[1]], b[i[0], 3 + i[1]], lo[i], hi[i]))
    # the leaves of the binary tree, box for box
    first = np.array([int(np.argmax(r)) if r.any() else -1 for r in m]); count = m.sum(1)
    contiguous = np.array([r[f:f + c].all() if f >= 0 else False for r, f, c in zip(m, first, count)])
    rep.where(~contiguous, "cover", lambda i: "flat leaf %d does not hold one run of records" % i[0])
    a = np.sort(_key(first, count)); k = np.sort(_key(binary["leaf_first"], binary["leaf_count"]))
    if a.size != np.unique(k).size or (a != np.unique(k)).any():
        rep.add("cover", "the flat list's leaves are not the binary tree's")
    found, bb = _lookup(binary, first, count)
    rep.where(found & (bb != box).any(1), "tightness", lambda i: "flat leaf %d: its box is not the binary tree's box of the same leaf" % i[0])


# ---- everything -------------------------------------------------------------------------------------------------------------------
def validate(tabs, info, input_prims=None, input_meta=None, max_leaf=16, device_built=False):
    """Every check of DESIGN.md "Tree tables, checked structurally" on one upload's tables.  input_prims (n, 16) float32 / input_meta (n, 4) int32: the records in
    the caller's primitive order.  device_built: extents as k_lbvh_bounds takes them, unreached binary nodes all-zero, child boxes no looser than the padded union;
    host-built: the caller's tree (every node reached; boxes are the caller's, so only containment is theirs to satisfy)."""
    rep = Report()
    get = lambda k: tabs.get(k) if tabs.get(k) is not None else EMPTY
    prims = decode_prims(get("prims")); meta = decode_meta(get("meta"))
    n = int(info["n_prims"])
    if prims.shape[0] != n or meta.shape[0] != n:
        rep.add("bounds", "%d primitive records, %d meta records, n_prims %d" % (prims.shape[0], meta.shape[0], n)); return rep
    # permutation
    idx = meta[:, 0].astype(np.int64)
    perm_ok = not rep.where((idx < 0) | (idx >= n), "permutation", lambda i: "meta[%d] names primitive %d of %d" % (i[0], idx[i[0]], n))
    if perm_ok:
        c = np.bincount(idx, minlength=n)
        perm_ok = not rep.where(c != 1, "permutation", lambda i: "the caller's primitive %d appears %d times" % (i[0], c[i[0]]))
    if perm_ok and input_prims is not None:
        rep.where((prims.view(np.uint32) != np.ascontiguousarray(input_prims, F).view(np.uint32)[idx]).any(1), "permutation", lambda i: "record %d is not the input record of primitive %d" % (i[0], idx[i[0]]))
        rep.where((meta != np.asarray(input_meta, np.int32)[idx]).any(1), "permutation", lambda i: "meta %d is not the input's of primitive %d" % (i[0], idx[i[0]]))
    elo, ehi = prim_extents(prims, "sphere" if device_built else "tight")
    binary = walk_binary(rep, get("nodes"), n, int(info["n_nodes"]), elo, ehi, max_leaf=max_leaf, dense=not device_built, tight=device_built)
    heights = {"bvh_height": binary["height"]}
    if get("q4").size:
        heights["q4_height"] = walk_q4(rep, get("q4"), n, int(info["n_q4"]), elo, ehi, binary, max_leaf=max_leaf)
    elif int(info["n_q4"]):
        rep.add("bounds", "n_q4 %d without a 4-wide table" % info["n_q4"])
    if get("wide").size:
        heights["wide_height"] = walk_wide8(rep, get("wide"), n, int(info["n_wide"]), elo, ehi, binary)
    elif int(info["n_wide"]):
        rep.add("bounds", "n_wide %d without an 8-wide table" % info["n_wide"])
    if get("flat").size:
        check_flat(rep, get("flat"), n, elo, ehi, binary)
    for k, real in heights.items():
        got = int(info[k])
        if got < real:
            rep.add("height", "%s %d UNDER-reports the real depth %d: the traversal stack sized from it overflows" % (k, got, real))
        elif got > real:
            rep.add("height", "%s %d over-reports the real depth %d" % (k, got, real))
    rep.stats = dict(heights, n_leaves=int(binary["leaf_first"].size))
    rep.binary = binary
    return rep


# ---- the exact LBVH reference -----------------------------------------------------------------------------------------------------
def _spread21(v):
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for sh, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(mask)
    return x


def morton_keys(input_prims):
    """the 63-bit keys of k_lbvh_morton for records in creation order, fp32 operation by operation (each a single correctly rounded IEEE operation)"""
    lo, hi = prim_extents(np.ascontiguousarray(input_prims, F), "sphere")
    lo = lo.astype(F); hi = hi.astype(F)
    sl = lo.min(0); sh = hi.max(0)
    c = F(0.5) * (lo + hi)
    ext = sh - sl
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ext > 0, (c - sl) / np.where(ext > 0, ext, F(1)), F(0)).astype(F)
    t = np.minimum(np.maximum(t, F(0)), F(1)) * F(2097152.0)
    q = np.minimum(t, F(2097151.0)).astype(np.uint32)
    return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])


def lbvh_reference(input_prims, max_leaf):
    """-> order (device position -> creation index), refs (n - 1, 2) int32 of the emitted nodes (zero rows where none is emitted), emitted mask.
    Karras 2012 top down over (key, position): a range splits below the highest bit in which its first and last (key, position) differ; the left part of a split
    at gamma is node gamma, the right part node gamma + 1; a part of at most max_leaf positions is a leaf; the root is always emitted."""
    keys = morton_keys(input_prims)
    order = np.argsort(keys, kind="stable")
    n = keys.size
    aug = [(int(k) << 32) | i for i, k in enumerate(keys[order])]
    refs = np.zeros((max(1, n - 1), 2), np.int32); emitted = np.zeros(max(1, n - 1), bool)
    if n < 2:
        return order, refs, emitted
    stack = [(0, 0, n - 1)]
    while stack:
        node, f, e = stack.pop()
        bit = (aug[f] ^ aug[e]).bit_length() - 1
        gamma = bisect.bisect_left(aug, ((aug[e] >> bit) << bit), f, e + 1) - 1
        emitted[node] = True
        for s, (cf, ce, cnode) in enumerate(((f, gamma, gamma), (gamma + 1, e, gamma + 1))):
            cnt = ce - cf + 1
            if cnt <= max_leaf:
                refs[node, s] = leaf_ref(cf, cnt)
            else:
                refs[node, s] = cnode; stack.append((cnode, cf, ce))
    return order, refs, emitted


# ---- the wide tables under a numbering of their own ----------------------------------------------------------------------------------------
# The device collapses allocate node indices with atomicAdd, so two builds of one tree may number the nodes of a level differently.  Renumbered breadth first
# (level by level, parents in order, slots in order) two tables of the same tree are byte-equal.  For tables that passed validate().
def _breadth_first(n, children_of):
    order = [np.array([0], np.int64)]
    while order[-1].size:
        order.append(children_of(order[-1]))
    order = np.concatenate(order)
    newid = np.full(n, -1, np.int64); newid[order] = np.arange(order.size)
    return order, newid


def canonical_q4(b):
    w = _words(b, 16, np.uint32)
    refs = w[:, 4:8].copy().view(np.int32).astype(np.int64)
    inner = (((w[:, 3] >> 24)[:, None] >> np.arange(4)) & 1).astype(bool) & (refs >= 0)
    order, newid = _breadth_first(w.shape[0], lambda f: refs[f][inner[f]])
    out = w[order].copy()
    r = refs[order]; r[inner[order]] = newid[r[inner[order]]]
    out[:, 4:8] = r.astype(np.int32).view(np.uint32)
    return out


def canonical_wide8(b):
    w = decode_wide8(b)
    meta = w["meta"]
    inner = (meta != 0) & ((meta & 0x18) == 0x18)
    child = w["child_base"][:, None] + np.cumsum(inner, axis=1) - inner
    order, newid = _breadth_first(meta.shape[0], lambda f: child[f][inner[f]])
    out = w["raw"][order].copy()
    has = inner[order].any(1)
    out[has, 4] = newid[w["child_base"][order][has]].astype(np.uint32)
    return out
