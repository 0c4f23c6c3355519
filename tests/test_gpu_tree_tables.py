"""The hierarchies the DEVICE builds (csrc/jp_lbvh.h: LBVH pipeline, radix sort, 8-wide and 4-wide collapses; csrc/jp_ploc.h: PLOC clustering and its scans), read
back with jp_read_scene_table and checked structurally by tests/tree_ref.py: partition, permutation, leaf sizes, containment, tightness, heights, the wide trees
covering the binary tree -- and, for the LBVH, equality with a plain Karras reference over bit-equal Morton keys.  Counts sit on the places where the kernels change
behaviour (256 threads per block, 1,024 elements per scan workgroup = the 4-wide threshold, 2,048 pairs per radix tile, the 64-primitive 8-wide threshold, the
second 256-chunk of k_scan2_tops above 262,144 clusters).  One upload and one numpy pass per case; nothing is rendered.  DESIGN.md "Tree tables, checked structurally"."""
import time

import numpy as np
import pytest

import jet_pbrt_amd as jp
import tree_ref as T
import tree_scenes as S
import test_upload_host as U

pytestmark = pytest.mark.gpu

COUNTS = [2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097]
TREES = {"ploc": 1, "lbvh": 2}
DEFAULT_LEAF = {"ploc": 2, "lbvh": 3}
LARGE = 270000                                                          # > 262,144: the first PLOC round scans 264 block totals, k_scan2_tops' second chunk


@pytest.fixture(scope="module")
def ctx():
    c = jp.Context(0)
    yield c
    c.close()


def build(ctx, sc, tree, **opts):
    """upload under device_tree = tree (and opts), back to the initial options afterwards -> (tabs, info, JpBuildInfo)"""
    ctx.set_options(device_tree=TREES[tree], **opts)
    try:
        ctx.upload(sc.ptr())
    finally:
        ctx.set_options()
    tabs, info = S.device_tables(ctx)
    return tabs, info, ctx.build_info()


def check(tabs, info, bi, sc, tree, max_leaf, wide_may_refuse=False):
    n = sc.n
    prims, meta = S.input_records(sc.scene)
    rep = T.validate(tabs, info, prims, meta, max_leaf=max_leaf, device_built=True)
    assert rep.ok(), str(rep)
    assert bi.built_on_device == 1 and info["n_prims"] == n and info["n_nodes"] == n - 1 and bi.bvh_height == info["bvh_height"]
    # which trees exist: no silent fallback at the default leaf size
    if n <= 64:
        assert info["n_wide"] == 0 and tabs["wide"].size == 0
    elif not wide_may_refuse:
        assert info["n_wide"] > 0, "the 8-wide collapse fell back to the binary tree"
    assert bi.traversal_mode == (3 if info["n_wide"] > 0 else 0)       # a refused collapse is what the build info reports
    assert (info["n_q4"] > 0) == (n > 1024), "the 4-wide collapse %s" % ("fell back to the binary tree" if n > 1024 else "ran below its threshold")
    assert bi.q4_nodes == info["n_q4"]
    assert tabs["flat"].size == 0
    if tree == "lbvh":
        order, refs, emitted = T.lbvh_reference(prims, max_leaf)
        got = T.decode_meta(tabs["meta"])[:, 0]
        assert (got == order).all(), "LBVH primitive order is not the stable sort of the Morton keys (first difference at position %d)" % int(np.argmax(got != order))
        _, grefs, raw = T.decode_binary(tabs["nodes"])
        assert ((raw != 0).any(1) == emitted).all(), "LBVH emits other nodes than the Karras reference"
        bad = (grefs != refs).any(1)
        assert not bad.any(), "LBVH node %d: refs %s, Karras reference %s" % (int(np.argmax(bad)), grefs[np.argmax(bad)], refs[np.argmax(bad)])
    return rep


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tree", sorted(TREES))
def test_device_trees_at_every_count(ctx, tree, n):
    sc = S.make(n, "uniform")
    check(*build(ctx, sc, tree), sc, tree, DEFAULT_LEAF[tree])


@pytest.mark.parametrize("n", [65, 1025, 2049])
@pytest.mark.parametrize("leaf", [1, 16])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_device_trees_at_other_leaf_sizes(ctx, tree, leaf, n):
    """bvh_max_leaf = 16: two 16-primitive leaves need twelve chunk slots, so the 8-wide collapse may refuse; the binary tree then serves and is what is validated"""
    sc = S.make(n, "uniform", seed=2)
    tabs, info, bi = build(ctx, sc, tree, bvh_max_leaf=leaf)
    rep = check(tabs, info, bi, sc, tree, leaf, wide_may_refuse=(leaf == 16))
    if leaf == 1:
        assert rep.stats["n_leaves"] == n


def test_ploc_with_the_narrowest_window(ctx):
    sc = S.make(1025, "uniform", seed=3)
    check(*build(ctx, sc, "ploc", ploc_radius=1), sc, "ploc", 2)


@pytest.mark.parametrize("n", [2049, 4097])
@pytest.mark.parametrize("dist", ["uniform", "coincident", "planar", "clusters", "cell"])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_device_trees_over_key_distributions(ctx, tree, dist, n):
    sc = S.make(n, dist, seed=4)
    prims, _ = S.input_records(sc.scene)
    keys = T.morton_keys(prims)
    if dist == "coincident":
        assert (keys == keys[0]).all()
    elif dist == "planar":
        assert ((keys & np.uint64(0x1249249249249249)) == 0).all()      # no extent along z: its bits are all 0
    elif dist == "clusters":
        assert np.unique(keys >> np.uint64(40)).size == 2 and np.unique(keys).size <= 128
    elif dist == "cell":
        assert np.unique(keys[2:] >> np.uint64(24)).size <= 8 and np.unique(keys[2:]).size > n // 2
    tabs, info, bi = build(ctx, sc, tree)
    check(tabs, info, bi, sc, tree, DEFAULT_LEAF[tree])
    if dist == "coincident" and tree == "lbvh":                         # equal keys: the sort's stability across waves and tiles is all that orders them
        assert (T.decode_meta(tabs["meta"])[:, 0] == np.arange(n)).all()


@pytest.mark.parametrize("tree", sorted(TREES))
def test_device_trees_large(ctx, tree):
    sc = S.make(LARGE, "uniform", seed=5)
    prims, meta = S.input_records(sc.scene)
    tabs, info, bi = build(ctx, sc, tree)
    t0 = time.perf_counter()
    rep = T.validate(tabs, info, prims, meta, max_leaf=DEFAULT_LEAF[tree], device_built=True)
    dt = time.perf_counter() - t0
    print("tree_ref.validate, %s, %d primitives: %.2f s; heights %s, build %.1f ms" % (tree, LARGE, dt, rep.stats, bi.device_build_ms))
    assert rep.ok(), str(rep)
    assert info["n_wide"] > 0 and info["n_q4"] > 0 and bi.traversal_mode == 3 and info["n_nodes"] == LARGE - 1


@pytest.mark.parametrize("tree", sorted(TREES))
def test_validator_bites_on_device_built_tables(ctx, tree):
    """the device-build rules of the validator on real device tables: a leaf above the limit, a child box three ulp too small (inside its pad: no primitive is
    lost yet), an under-reported height, a wrapped leaf's node dropped from the 8-wide tree"""
    leaf = DEFAULT_LEAF[tree]
    sc = S.make(1025, "uniform", seed=8)
    prims, meta = S.input_records(sc.scene)
    tabs, info, _ = build(ctx, sc, tree)
    assert T.validate(tabs, info, prims, meta, max_leaf=leaf, device_built=True).ok()
    assert T.validate(tabs, info, prims, meta, max_leaf=leaf - 1, device_built=True).kinds() == {"leaf_size"}
    t2 = {k: v.copy() for k, v in tabs.items()}
    nd = t2["nodes"].view(np.float32).reshape(-1, 16)
    node = int(np.flatnonzero((t2["nodes"].view(np.uint32).reshape(-1, 16) != 0).any(1))[-1])
    for _ in range(3):
        nd[node, 0] = np.nextafter(nd[node, 0], np.float32(np.inf))
    rep = T.validate(t2, info, prims, meta, max_leaf=leaf, device_built=True)
    assert any(k == "tightness" and "binary node %d child 0 axis 0" % node in m and "tighter" in m for k, m in rep.errors), str(rep)
    for f in ("bvh_height", "wide_height", "q4_height"):
        rep = T.validate(tabs, dict(info, **{f: info[f] - 1}), prims, meta, max_leaf=leaf, device_built=True)
        assert [k for k, _ in rep.errors] == ["height"] and "UNDER-reports" in rep.errors[0][1]
    t2 = {k: v.copy() for k, v in tabs.items()}
    w = t2["wide"].view(np.uint32).reshape(-1, 20)
    imask = int(w[0, 3]) >> 24
    top = imask.bit_length() - 1                                        # the root's last inner child: mask bit and meta byte go, its subtree is cut off
    w[0, 3] = (int(w[0, 3]) & 0x00ffffff) | ((imask & ~(1 << top)) << 24)
    t2["wide"].view(np.uint8).reshape(-1, 80)[0, 24 + top] = 0
    rep = T.validate(t2, info, prims, meta, max_leaf=leaf, device_built=True)
    assert "partition" in rep.kinds(), str(rep)


@pytest.mark.parametrize("tree", sorted(TREES))
def test_device_trees_are_a_function_of_the_input(ctx, tree):
    """twice in one context, once in a fresh one: nodes, prims and meta byte for byte; the wide tables after renumbering (their indices come from atomicAdd order)"""
    sc = S.make(4097, "uniform", seed=6)
    other = S.make(1025, "uniform", seed=7)
    a, ia, _ = build(ctx, sc, tree)
    build(ctx, other, tree)
    b, ib, _ = build(ctx, sc, tree)
    fresh = jp.Context(0)
    try:
        c, ic, _ = build(fresh, sc, tree)
    finally:
        fresh.close()
    assert T.validate(a, ia, device_built=True, max_leaf=DEFAULT_LEAF[tree]).ok()
    for x, ix in ((b, ib), (c, ic)):
        assert ix == ia
        for k in ("nodes", "prims", "meta"):
            assert np.array_equal(a[k], x[k]), k
        assert np.array_equal(T.canonical_q4(a["q4"]), T.canonical_q4(x["q4"]))
        assert np.array_equal(T.canonical_wide8(a["wide"]), T.canonical_wide8(x["wide"]))


def test_host_built_tables_arrive_on_the_device_unchanged(ctx, tmp_path):
    be, sp, _, mode = U.build_case("random_1600", tmp_path)
    try:
        ctx.set_light_sampling(mode)
        ctx.upload(sp)
        o = ctx.get_options()
        d = jp.describe_upload(sp, o, mode)
        tabs, info = S.device_tables(ctx)
        for k in S.TABLES:
            assert np.array_equal(tabs[k], jp.copy_upload_table(sp, k, o, mode)), k
        assert info == {f: int(getattr(d, f)) for f in S.INFO_FIELDS} and tabs["wide"].size and tabs["q4"].size
        assert ctx.build_info().built_on_device == 0
        with pytest.raises(jp.JetPbrtError):
            ctx.read_table("mats")
    finally:
        be.close()
