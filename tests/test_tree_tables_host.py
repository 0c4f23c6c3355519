"""The host-built hierarchy tables (csrc/jp_scene_host.h: binary, 8-wide, 4-wide, flat) are WELL-FORMED, not merely unchanged: jp_copy_upload_table hands back the
bytes jp_describe_upload hashes, tests/tree_ref.py decodes them in plain numpy and checks partition, permutation, leaf sizes, containment, quantisation tightness,
heights and that the wide trees cover the binary tree (DESIGN.md "Tree tables, checked structurally").  No GPU needed.  The validator itself is shown to bite."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import tree_ref as T
import tree_scenes as S
import test_upload_host as U

HOST_CASES = sorted(n for n, c in U.CASES.items() if c[1] is None)      # the reference-tree cases keep their own tests: their node table is the caller's, verbatim
THRESHOLDS = [63, 64, 65, 1023, 1024, 1025]                            # 64: flat list / 8-wide; 1024: 4-wide


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return tmp_path_factory.mktemp("tree_host")


def _validate(sp, options=None, mode="all"):
    tabs, info, full = S.host_tables(sp, options, mode)
    prims, meta = S.input_records(sp)
    rep = T.validate(tabs, info, prims, meta, max_leaf=16, device_built=False)
    return tabs, info, full, rep


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_copied_tables_are_the_bytes_describe_upload_hashes(name, tmpdir):
    """all eleven tables: same byte count, same FNV-1a (computed here) as JpUploadInfo reports, so the two entry points cannot drift"""
    be, sp, o, mode = U.build_case(name, tmpdir)
    info = jp.describe_upload(sp, o, mode)
    for k, tab in enumerate(jp.UPLOAD_TABLES):
        b = jp.copy_upload_table(sp, tab, o, mode)
        assert b.size == info.table[k].bytes, tab
        assert (S.fnv1a(b) if b.size else 0) == info.table[k].fnv1a, tab
    be.close()


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_tables_of_the_upload_cases_are_valid_trees(name, tmpdir):
    be, sp, o, mode = U.build_case(name, tmpdir)
    tabs, info, full, rep = _validate(sp, o, mode)
    assert rep.ok(), str(rep)
    # the walk saw what the plan says there is
    assert (tabs["wide"].size > 0) == (full.n_wide > 0) and (tabs["q4"].size > 0) == (full.n_q4 > 0) == bool(full.use_q4) and (tabs["flat"].size > 0) == (full.n_flat > 0)
    assert rep.stats["n_leaves"] >= 2
    be.close()


@pytest.mark.parametrize("n", THRESHOLDS)
def test_host_tables_at_the_table_thresholds(n, tmpdir):
    be = S.host_backend(n, tmpdir)
    sp = be.flatten()
    tabs, info, full, rep = _validate(sp)
    assert rep.ok(), str(rep)
    assert info["n_prims"] == n
    assert (full.n_q4 > 0) == (n > 1024)                                # the 4-wide tree exists exactly above its threshold
    assert (full.n_flat > 0) <= (n <= 64)                               # the flat list never above its own
    assert (full.n_wide > 0) == (full.trav_mode == 3) == (n >= 1023)    # the 8-wide tree: scenes past the 40 KB of LDS the binary tree may take (80 bytes per node and record)
    be.close()


def test_copy_upload_table_arguments(tmpdir):
    L = jp.hip_lib()
    be, s = U._cornell()
    n = C.c_int64(-1)
    assert L.jp_copy_upload_table(None, 0, C.byref(s), 0, None, 0, C.byref(n)) == 0 and n.value > 0 and n.value % 64 == 0     # out NULL: the size only
    buf = np.zeros(n.value, np.uint8)
    assert L.jp_copy_upload_table(None, 0, C.byref(s), 0, buf.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n)) == U.INVALID and not buf.any()
    assert L.jp_copy_upload_table(None, 0, C.byref(s), 11, None, 0, C.byref(n)) == U.INVALID and L.jp_copy_upload_table(None, 0, C.byref(s), -1, None, 0, C.byref(n)) == U.INVALID
    assert L.jp_copy_upload_table(None, 0, None, 0, None, 0, C.byref(n)) == U.INVALID and L.jp_copy_upload_table(None, 0, C.byref(s), 0, None, 0, None) == U.INVALID
    assert L.jp_copy_upload_table(None, 0, C.byref(s), jp.UPLOAD_TABLES.index("q4"), None, 0, C.byref(n)) == 0 and n.value == 0   # a table this upload does not have
    s.n_bvh_nodes = 0
    assert L.jp_copy_upload_table(None, 0, C.byref(s), 0, None, 0, C.byref(n)) == U.UNSUPPORTED
    be.close()


# ---- the validator bites: one valid table set, five corruptions, each reported ----------------------------------------------------------
@pytest.fixture(scope="module")
def valid_set(tmpdir):
    """the 1,025-primitive host scene: binary, 8-wide and 4-wide trees at once"""
    be = S.host_backend(1025, tmpdir)
    sp = be.flatten()
    tabs, info, full = S.host_tables(sp)
    prims, meta = S.input_records(sp)
    assert tabs["wide"].size and tabs["q4"].size
    assert T.validate(tabs, info, prims, meta).ok()
    yield tabs, info, prims, meta
    be.close()


def _corrupt(valid_set, table=None):
    tabs, info, prims, meta = valid_set
    tabs = {k: v.copy() for k, v in tabs.items()}
    return tabs, dict(info), prims, meta


def test_validator_reports_a_shrunk_plane_byte(valid_set):
    for name, words, first_plane, slots in (("q4", 16, 8, 4), ("wide", 20, 8, 8)):
        tabs, info, prims, meta = _corrupt(valid_set)
        raw = tabs[name].view(np.uint8).reshape(-1, 4 * words)
        hi = raw[:, 4 * first_plane + 3 * slots:4 * first_plane + 4 * slots]      # the hi-x bytes of every node
        lo = raw[:, 4 * first_plane:4 * first_plane + slots]
        node, slot = np.argwhere((hi > lo) & (hi > 0))[-1]                 # a live slot deep in the table
        hi[node, slot] -= 1
        rep = T.validate(tabs, info, prims, meta)
        assert "containment" in rep.kinds(), (name, str(rep))
        assert any("%s node %d" % ("4-wide" if name == "q4" else "8-wide", node) in m for k, m in rep.errors if k == "containment")


def test_validator_reports_a_duplicated_leaf_ref(valid_set):
    tabs, info, prims, meta = _corrupt(valid_set)
    refs = tabs["nodes"].view(np.int32).reshape(-1, 16)[:, 12:14]
    leaves = np.argwhere(refs < 0)
    (a, sa), (b, sb) = leaves[3], leaves[-2]
    refs[b, sb] = refs[a, sa]
    rep = T.validate(tabs, info, prims, meta)
    assert "partition" in rep.kinds(), str(rep)
    assert any(k == "partition" and "binary leaves" in m for k, m in rep.errors)       # (one position twice, another not at all; the first offender is named)
    assert "cover" in rep.kinds()                                       # ... and the wide trees no longer hold the binary tree's leaves


def test_validator_reports_a_dropped_chunk_bit(valid_set):
    tabs, info, prims, meta = _corrupt(valid_set)
    mb = tabs["wide"].view(np.uint8).reshape(-1, 80)[:, 24:32]
    chunk = (mb != 0) & ((mb & 0x18) != 0x18)
    node, slot = np.argwhere(chunk & ((mb >> 5) >= 3))[0]                # a chunk of two or three primitives loses its last one: unary 0b11 -> 0b01, 0b111 -> 0b011
    mb[node, slot] = ((mb[node, slot] >> 6) << 5) | (mb[node, slot] & 31)
    rep = T.validate(tabs, info, prims, meta)
    assert any(k == "partition" and "is in 0 8-wide leaf chunks" in m for k, m in rep.errors), str(rep)


def test_validator_reports_a_reference_past_the_end(valid_set):
    # a child index past the node table, in each tree; and a leaf range past the records
    tabs, info, prims, meta = _corrupt(valid_set)
    refs = tabs["nodes"].view(np.int32).reshape(-1, 16)[:, 12:14]
    node, side = np.argwhere(refs >= 0)[-1]
    refs[node, side] = info["n_nodes"]
    rep = T.validate(tabs, info, prims, meta)
    assert any(k == "bounds" and "past n_nodes" in m for k, m in rep.errors), str(rep)
    tabs, info, prims, meta = _corrupt(valid_set)
    refs = tabs["nodes"].view(np.int32).reshape(-1, 16)[:, 12:14]
    node, side = np.argwhere(refs < 0)[-1]
    refs[node, side] = int(T.leaf_ref(info["n_prims"] - 1, 2))
    rep = T.validate(tabs, info, prims, meta)
    assert any(k == "bounds" and "n_prims" in m for k, m in rep.errors), str(rep)
    tabs, info, prims, meta = _corrupt(valid_set)
    q = tabs["q4"].view(np.int32).reshape(-1, 16)
    node, slot = np.argwhere(q[:, 4:8] > 0)[-1]
    q[node, 4 + slot] = info["n_q4"]
    rep = T.validate(tabs, info, prims, meta)
    assert any(k == "bounds" and "4-wide child index" in m for k, m in rep.errors), str(rep)
    tabs, info, prims, meta = _corrupt(valid_set)
    w = tabs["wide"].view(np.uint32).reshape(-1, 20)
    node = int(np.flatnonzero((w[:, 3] >> 24) != 0)[-1])
    w[node, 4] = info["n_wide"]
    rep = T.validate(tabs, info, prims, meta)
    assert any(k == "bounds" and "8-wide child index" in m for k, m in rep.errors), str(rep)


@pytest.mark.parametrize("field", ["bvh_height", "wide_height", "q4_height"])
def test_validator_reports_a_height_one_too_low(valid_set, field):
    tabs, info, prims, meta = _corrupt(valid_set)
    info[field] -= 1
    rep = T.validate(tabs, info, prims, meta)
    assert [k for k, _ in rep.errors] == ["height"] and "UNDER-reports" in rep.errors[0][1] and field in rep.errors[0][1], str(rep)
    info[field] += 2
    rep = T.validate(tabs, info, prims, meta)
    assert [k for k, _ in rep.errors] == ["height"] and "over-reports" in rep.errors[0][1]


def test_validator_reports_a_loose_box_and_a_swapped_record(valid_set):
    """the other two defects a random ray set cannot see: a quantised box far too loose, and a record that is not its primitive's"""
    tabs, info, prims, meta = _corrupt(valid_set)
    raw = tabs["q4"].view(np.uint8).reshape(-1, 64)
    hi = raw[:, 32 + 12:32 + 16]
    node, slot = np.argwhere((hi > 0) & (hi < 200))[-1]
    hi[node, slot] = 255
    assert "tightness" in T.validate(tabs, info, prims, meta).kinds()
    tabs, info, prims, meta = _corrupt(valid_set)
    m = tabs["meta"].view(np.int32).reshape(-1, 4)
    m[[5, 6], 0] = m[[6, 5], 0]
    assert "permutation" in T.validate(tabs, info, prims, meta).kinds()


# ---- the exact LBVH reference agrees with itself on a hand-checkable case -------------------------------------------------------------------
def test_lbvh_reference_on_a_line_of_spheres():
    """eight unit-spaced spheres along x: keys ascend with x, and the Karras splits of eight consecutive codes 0 .. 7 scaled are the balanced tree"""
    g = np.zeros((8, 16), np.float32)
    g[:, 0] = np.arange(8)[::-1]; g[:, 3] = 0.25; g.view(np.int32)[:, 15] = T.SPHERE
    keys = T.morton_keys(g)
    assert (np.diff(keys[::-1].astype(np.int64)) > 0).all()
    order, refs, emitted = T.lbvh_reference(g, 1)
    assert order.tolist() == list(range(7, -1, -1))
    assert emitted.all()
    first, count = T.leaf_range(refs[refs < 0])
    assert sorted(first.tolist()) == list(range(8)) and (count == 1).all()
    order, refs, emitted = T.lbvh_reference(g, 2)
    first, count = T.leaf_range(refs[emitted][refs[emitted] < 0])
    assert sorted(zip(first.tolist(), count.tolist())) == [(0, 2), (2, 2), (4, 2), (6, 2)] and emitted.sum() == 3


def test_tree_info_layout_matches_header(tmp_path):
    """the ctypes mirror of JpTreeInfo has the C layout, and JpBuildInfo kept its size (the wide heights went into a struct of their own)"""
    import os
    import subprocess
    src = ('#include "jetpbrt_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){ printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(JpTreeInfo), offsetof(JpTreeInfo, wide_height), '
           'offsetof(JpTreeInfo, n_flat), sizeof(JpBuildInfo), JP_TABLE_NODES, JP_TABLE_PRIMS, JP_TABLE_META, JP_TABLE_WIDE, JP_TABLE_Q4, JP_TABLE_FLAT); return 0; }')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(U.H.REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    I = jp.JpTreeInfo
    assert out == [C.sizeof(I), I.wide_height.offset, I.n_flat.offset, 64] + [jp.UPLOAD_TABLES.index(k) for k in ("nodes", "prims", "meta", "wide", "q4", "flat")]
    assert C.sizeof(jp.JpBuildInfo) == 64
