"""The any-hit half of every traversal structure, ray by ray (jp_occluded: k_occluded<mode>, SceneAccess<mode>::trace<true> -- what the render's shadow rays
run one ray per lane).  The scenes, ray sets and their float64 results are those of tests/rays_sets.py / tests/rays_ref.py, which tests/test_rays_host.py
pins to the fp32 CPU oracle without a GPU.  Per scene, per row of the table below (one upload each) and per forced walk:

  A  same structure, both queries: `occluded` is 0 or 1 and equals jp_trace's `hit` under the same options on EVERY ray.  Exact, not statistical: both queries
     run the same primitive test, every box test is monotone in tmax, and the closest-hit walk only shrinks tmax once it has a hit -- so a leaf either query
     reaches with an accepted primitive is reached, or made moot by an earlier hit, in the other.  The exact-t set (tmax = the fp32 t jp_trace returned, and
     its two neighbours) and the non-decisive rays matter most here.
  B  against float64: on decisive rays `occluded` and jp_trace's `hit` equal the reference's verdict; where the nearest hit is beyond doubt and unique,
     jp_trace's primitive is that one and |t - t64| <= T_TOL * max(|t|, S).
  C  across structures: on decisive rays all rows of a scene agree; the certified walk equals the verbatim walk on every ray.
  D  housekeeping: error codes, n == 0, device memory, repeatability, a render before and after.

Every row asserts through walk_out that the walk it names ran (mode, + 16 for the flat-shape instance).  The lane-refill kernels (k_shadow_persist) drive the
same Walker steps with several rays per lane; their equality with the one-ray-per-lane kernels stays with
test_wavefront_sorts_and_lane_refill_do_not_change_the_film."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import rays_ref as R
import rays_sets as RS

pytestmark = pytest.mark.gpu
JP_ERR_INVALID_ARGUMENT, JP_ERR_NO_SCENE = -1, -4
LEAN = 2 + 16
GENERIC = dict(reserved=(C.c_int32 * 8)(1))

# scene -> rows (tag, tree handed over, options of the upload, calls); a call is (trace_walk, the walk jp_occluded must report, jp_trace is on that structure too)
_FLAT = [("lean", "host", {}, [(0, LEAN, True)]), ("generic", "host", GENERIC, [(0, 2, True)])]
_CURVED = [("generic", "host", {}, [(0, 2, True)])]
_ALL3 = [(0, 4, True), (1, 0, True), (2, 3, True)]
ROWS = {
    "cornell": _FLAT + [("lds", "host", dict(traversal=2), [(0, 1, True)]), ("binary", "host", dict(traversal=1), [(0, 0, True)])],
    "misc": _CURVED, "disks": _CURVED,
    "lights": _FLAT,                                                     # (the Cornell box under delta lights: flat shapes only, so the flat-shape instance)
    RS.LARGE: [("q4", "host", {}, _ALL3),
               ("wide", "host", dict(q4_shadow=-1), [(0, 3, False), (2, 3, True)]),      # shadow rays on the 8-wide tree; jp_trace joins them there under trace_walk 2
               ("binary", "host", dict(traversal=1, q4=-1), [(0, 0, True)]),
               ("ploc", "device", dict(device_tree=1), _ALL3), ("lbvh", "device", dict(device_tree=2), _ALL3)],
    "bunny_small": [("verbatim", "reference", {}, [(0, 5, True)]), ("certified", "certified", {}, [(0, 6, True), (3, 5, True)])],
    "one_triangle": _FLAT, "one_rectangle": _FLAT, "tri32": _FLAT, "tri33": _FLAT,
    "one_sphere": _CURVED, "one_disk": _CURVED, "two": _CURVED, "all_lights": _CURVED,
}
# rays a check of this file once failed on, kept: scene -> (o, d, tmin, tmax) rows (none so far: A, B and C held on the first run)
PINNED = {}


@pytest.fixture(scope="module")
def ctx():
    c = jp.Context(0)
    yield c
    c.close()


def _show(rays, i):
    return [a[i].tolist() for a in rays]


def _exact_t(ctx, rays):
    """far ends on and beside the fp32 distance jp_trace returns on the structure in force: non-decisive by construction"""
    o, d, tmin, _ = (a[:1501] for a in rays)
    hit, t, _, _ = ctx.trace(o, d, tmin, np.full(len(o), np.inf, np.float32))
    k = hit != 0
    o, d, tmin, t = o[k], d[k], tmin[k], t[k]
    below, above = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    return np.concatenate([o, o, o]), np.concatenate([d, d, d]), np.concatenate([tmin, tmin, tmin]), np.concatenate([t, below, above])


def _check_calls(ctx, name, tag, calls, verdicts):
    sh = RS.shapes(name)
    sets = dict(RS.ray_sets(name))
    if name in PINNED:
        sets["pinned"] = tuple(np.asarray(a, np.float32) for a in PINNED[name])
    for tw, want, same in calls:
        ctx.set_options(trace_walk=tw)
        for which, rays in list(sets.items()) + [("exact_t", None)]:
            if which == "exact_t":
                if not same:
                    continue
                rays = _exact_t(ctx, sets["random"])
                if len(rays[0]) == 0:
                    continue
            occ, walk = ctx.occluded(*rays)
            assert walk == want, (name, tag, tw, "jp_occluded ran walk %d, the row names %d" % (walk, want))
            assert ((occ == 0) | (occ == 1)).all()
            hit, t, prim, _ = ctx.trace(*rays)
            if same:                                                       # A
                bad = np.nonzero(occ != hit)[0]
                assert len(bad) == 0, (name, tag, tw, which, "%d of %d rays: occluded != jp_trace's hit" % (len(bad), len(occ)), int(bad[0]), _show(rays, bad[0]), int(occ[bad[0]]))
            if which == "exact_t":
                n3 = len(occ) // 3
                # (tmax == t and below: `distance < tmax` fails for the hit itself, another primitive may still block -- A has said what there is to say)
                assert occ[2 * n3:].all(), (name, tag, tw, "a far end one ulp behind the hit's own fp32 t")
                continue
            if which == "pinned":
                continue
            ref = RS.reference(name, which)                                # B
            dec = ref["decisive"]
            for what, got in (("occluded", occ), ("jp_trace", hit)):
                bad = np.nonzero(dec & ((got != 0) != ref["hit"]))[0]
                assert len(bad) == 0, (name, tag, tw, which, "%s differs from the float64 verdict on %d decisive rays" % (what, len(bad)), int(bad[0]), _show(rays, bad[0]), bool(ref["hit"][bad[0]]))
            uq = ref["unique"] & dec
            assert np.array_equal(prim[uq], ref["prim"][uq]), (name, tag, tw, which, int((prim[uq] != ref["prim"][uq]).sum()))
            err = np.abs(t[uq].astype(np.float64) - ref["t"][uq]) / np.maximum(np.abs(ref["t"][uq]), sh.S)
            cls = R.shape_class(sh, ref["prim"][uq])
            for k, tol in R.T_TOL.items():
                assert not (cls == k).any() or err[cls == k].max() <= tol, (name, tag, tw, which, k, float(err[cls == k].max()), tol)
            verdicts[(tag, tw, which)] = occ
    ctx.set_options(trace_walk=0)


@pytest.mark.parametrize("name", list(ROWS))
def test_occluded_on_every_walk(ctx, name):
    verdicts = {}
    try:
        for tag, tree, opts, calls in ROWS[name]:
            hb, sp = RS.build(name, tree)
            ctx.set_options()
            if opts:
                ctx.set_options(**opts)
            ctx.upload(sp)
            _check_calls(ctx, name, tag, calls, verdicts)
    finally:
        ctx.set_options()
    # C: all rows agree on the decisive rays (each equals the float64 verdict there); the same kernel under two options, and the certified walk against the
    # verbatim one, agree on every ray
    for which in RS.ray_sets(name):
        dec = RS.reference(name, which)["decisive"]
        rows = [(k, v) for k, v in verdicts.items() if k[2] == which]
        assert len(rows) == sum(len(calls) for _, _, _, calls in ROWS[name])
        for k, v in rows[1:]:
            assert np.array_equal(v[dec], rows[0][1][dec]), (name, which, rows[0][0], k)
        if name == RS.LARGE:
            assert np.array_equal(verdicts[("wide", 0, which)], verdicts[("wide", 2, which)])
        if name == "bunny_small":
            for k in (("certified", 3, which), ("verbatim", 0, which)):
                bad = np.nonzero(verdicts[("certified", 0, which)] != verdicts[k])[0]
                assert len(bad) == 0, (which, k, "the certified walk differs from the verbatim walk on %d rays" % len(bad), int(bad[0]), _show(RS.ray_sets(name)[which], bad[0]))


def test_bracket_sets_are_what_they_say(ctx):
    """the far end 4 m' before a decisive nearest hit: visible; 4 m' behind it: occluded -- on the default walk of the large scene and of the Cornell box"""
    for name in ("cornell", RS.LARGE):
        hb, sp = RS.build(name)
        ctx.upload(sp)
        for which, want in (("near", 0), ("far", 1)):
            dec = RS.reference(name, which)["decisive"]
            occ, _ = ctx.occluded(*RS.ray_sets(name)[which])
            assert dec.mean() > 0.98 and (occ[dec] == want).all(), (name, which)


def test_housekeeping(ctx):
    lib = ctx.lib
    hb, sp = RS.build("cornell")
    rays = RS.ray_sets("cornell")["random"]
    n = len(rays[0])
    occ = np.zeros(n, np.int32); walk = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(a) for a in rays] + [p(occ)]
    fresh = jp.Context(0)
    try:
        assert lib.jp_occluded(fresh.h, n, *args, C.byref(walk)) == JP_ERR_NO_SCENE and b"jp_occluded" in lib.jp_last_error()
    finally:
        fresh.close()
    ctx.upload(sp)
    assert lib.jp_occluded(None, n, *args, C.byref(walk)) == JP_ERR_INVALID_ARGUMENT
    assert lib.jp_occluded(ctx.h, -1, *args, C.byref(walk)) == JP_ERR_INVALID_ARGUMENT
    for i in range(len(args)):
        broken = list(args); broken[i] = None
        assert lib.jp_occluded(ctx.h, n, *broken, C.byref(walk)) == JP_ERR_INVALID_ARGUMENT, i
    assert walk.value == -7                                                # no refused call wrote it
    assert lib.jp_occluded(ctx.h, 0, *args, C.byref(walk)) == jp.JP_OK and walk.value == LEAN and not occ.any()
    assert lib.jp_occluded(ctx.h, n, *args, None) == jp.JP_OK and occ.any()     # walk_out may be NULL
    # device memory: the per-call scratch is gone after the call; two calls give the same array
    b0 = jp.device_bytes_in_use()
    a1, w1 = ctx.occluded(*rays)
    assert jp.device_bytes_in_use() == b0
    a2, w2 = ctx.occluded(*rays)
    assert jp.device_bytes_in_use() == b0 and np.array_equal(a1, a2) and w1 == w2 == LEAN and np.array_equal(a1, occ)
    # a render after the hook's calls equals one made before them
    params = jp.render_params(48, 48, 4, 5, 1234)
    ctx.upload(sp)
    before = ctx.render(params); c0 = ctx.counters()
    for which in ("random", "shadow", "edges"):
        ctx.occluded(*RS.ray_sets("cornell")[which])
    after = ctx.render(params); c1 = ctx.counters()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert (c0.shadow_rays, c0.shadow_occluded, c0.closest_rays) == (c1.shadow_rays, c1.shadow_occluded, c1.closest_rays)
