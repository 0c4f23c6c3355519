"""Vertex normals without a GPU (INTEGRATION.md "Vertex normals"): jp_interpolate_normals -- the function the device runs -- against the restatement of
tests/normals_ref.py bit for bit, its two special cases, the validation of jp_set_vertex_normals, the OBJ reader's vn field, the computed normals of
FScene::CreateTriangleMesh, the flattened normals and the struct layout."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import normals_ref as R

f32 = np.float32


def _triangles(rng, n):
    """n triangles whose angles are all >= 30 degrees, with unit normals tilted up to 40 degrees off Ng"""
    out = []
    while len(out) < n:
        p = rng.uniform(-2, 2, (3, 3))
        e = [p[(k + 1) % 3] - p[k] for k in range(3)]
        ang = [np.degrees(np.arccos(np.clip(-(e[k] @ e[k - 1]) / (np.linalg.norm(e[k]) * np.linalg.norm(e[k - 1])), -1, 1))) for k in range(3)]
        if min(ang) >= 30.0:
            out.append(p)
    p = np.array(out)
    ng = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]); ng /= np.linalg.norm(ng, axis=-1, keepdims=True)
    vn = np.zeros((n, 3, 3))
    for t in range(n):
        for k in range(3):
            v = rng.normal(size=3); v -= (v @ ng[t]) * ng[t]; v /= np.linalg.norm(v)
            a = np.radians(rng.uniform(0, 40))
            vn[t, k] = np.cos(a) * ng[t] + np.sin(a) * v
    return p.astype(f32), ng.astype(f32), vn.reshape(n, 9).astype(f32)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(7)
    p, ng, vn = _triangles(rng, 8)
    t = np.repeat(np.arange(8), 512)
    b = rng.dirichlet((1, 1, 1), len(t))
    pt = (b[:, :1] * p[t, 0] + b[:, 1:2] * p[t, 1] + b[:, 2:] * p[t, 2]).astype(f32)
    return p[t, 0], p[t, 1], p[t, 2], ng[t], vn[t], pt


def test_interpolation_is_the_definition_bit_for_bit(cases):
    got = jp.interpolate_normals(*cases)
    ref = R.interpolate32(*cases)
    assert len(got) == 4096 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_interpolation_is_close_to_float64(cases):
    got = jp.interpolate_normals(*cases).astype(np.float64)
    err = np.abs(got - R.interpolate64(*cases)).max()
    print("largest |fp32 - fp64| component: %.3e" % err)
    assert err <= 1e-4
    assert np.abs(np.linalg.norm(got, axis=-1) - 1.0).max() <= 1e-6


def test_zero_interpolant_falls_back_to_ng():
    a = lambda *v: np.array([v], f32)
    vn = np.array([[0, 0, 1, 0, 0, -1, 0, 1, 0]], f32)
    ng = a(0, 0, 1)
    got = jp.interpolate_normals(a(0, 0, 0), a(2, 0, 0), a(0, 2, 0), ng, vn, a(1, 0, 0))
    b0, b1, b2 = R.barycentrics(a(0, 0, 0), a(2, 0, 0), a(0, 2, 0), a(1, 0, 0), np.float32)
    assert (b0[0], b1[0], b2[0]) == (0.5, 0.5, 0.0)
    assert np.array_equal(got, ng)


def test_interpolant_is_flipped_onto_ngs_side():
    a = lambda *v: np.array([v], f32)
    n = np.array([0.6, 0.0, -0.8], f32)
    vn = np.concatenate([n, n, n])[None]
    got = jp.interpolate_normals(a(0, 0, 0), a(2, 0, 0), a(0, 2, 0), a(0, 0, 1), vn, a(0.5, 0.5, 0))
    assert got[0, 2] > 0 and np.allclose(got[0], -n, atol=1e-6)
    assert np.array_equal(got, R.interpolate32(a(0, 0, 0), a(2, 0, 0), a(0, 2, 0), a(0, 0, 1), vn, a(0.5, 0.5, 0)))


def test_validation_refuses_bad_normals_with_a_message():
    good = np.array([[0, 0, 1, 0, 0, 1, 0, 0, 1], [0] * 9], f32)
    assert jp.check_vertex_normals(good) == 1
    assert jp.check_vertex_normals(np.zeros((0, 9), f32)) == 0
    bad_nan = good.copy(); bad_nan[0, 4] = np.nan
    bad_long = good.copy(); bad_long[0, 3:6] = (0, 0, 2)
    bad_partial = good.copy(); bad_partial[1, 5] = 1.0
    for bad, word in ((bad_nan, "finite"), (bad_long, "length"), (bad_partial, "length")):
        with pytest.raises(jp.JetPbrtError) as e:
            jp.check_vertex_normals(bad)
        assert "status -1" in str(e.value) and word in str(e.value) and "triangle" in str(e.value)
    # lengths just inside 0.9 .. 1.1 pass, just outside do not
    edge = good.copy(); edge[0, 0:3] = (0, 0, 0.901); edge[0, 3:6] = (0, 0, 1.099)
    assert jp.check_vertex_normals(edge) == 1
    for bad_len in (0.899, 1.101):
        edge[0, 0:3] = (0, 0, bad_len)
        with pytest.raises(jp.JetPbrtError):
            jp.check_vertex_normals(edge)


def test_struct_sizes_match_the_header(H):
    src = r'''
    #include "jetpbrt_amd.h"
    #include <stdio.h>
    #include <stddef.h>
    int main(){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(JpVertexNormals), offsetof(JpVertexNormals, tri_vn), sizeof(JpNormalInfo),
                offsetof(JpNormalInfo, table_bytes_device), offsetof(JpNormalInfo, smooth_last_render), offsetof(JpNormalInfo, normal_ms)); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(jp.JpVertexNormals), jp.JpVertexNormals.tri_vn.offset, C.sizeof(jp.JpNormalInfo),
                                     jp.JpNormalInfo.table_bytes_device.offset, jp.JpNormalInfo.smooth_last_render.offset, jp.JpNormalInfo.normal_ms.offset]


# ---- the host API: OBJ reader, computed normals, flattening ---------------------------------------------------------------------------------------
def _write(name, text):
    p = os.path.join(scenes.asset_dir(), name)
    with open(p + ".tmp%d" % os.getpid(), "w") as fh:
        fh.write(text)
    os.replace(p + ".tmp%d" % os.getpid(), p)
    return p


def _flat_normals(be):
    """(tri_p0, tri_p1, tri_p2, tri_n, tri_vn or None) of a preprocessed host scene"""
    s = be.flatten().contents
    n = s.n_triangles
    arr = lambda ptr, k: np.ctypeslib.as_array(ptr, (n * k,)).reshape(n, k).copy()
    v = be.flatten_normals()
    vn = None if v is None else np.ctypeslib.as_array(v.tri_vn, (v.n_triangles * 9,)).reshape(v.n_triangles, 9).copy()
    return arr(s.tri_p0, 3), arr(s.tri_p1, 3), arr(s.tri_p2, 3), arr(s.tri_n, 3), vn


def _mesh_scene(path, smooth, flip_normal=False, flip_hand=False):
    be = scenes.HostBackend("normals_host")
    be.camera((0, -4, 0), (0, 1, 0), (0, 0, 1), 40.0, 8, 8)
    be.mesh(path, flip_normal, flip_hand, mat=be.mat_matte((0.5, 0.5, 0.5)), smooth=smooth)
    be.preprocess()
    return be


OBJ_VN = """o t
v 0 0 0
v 2 0 0
v 0 2 0
v 2 2 1
vt 0 0
vt 1 0
vt 0 1
vn 0 0 1
vn 0.6 0 0.8
vn 0 0.6 0.8
f 1/1/1 2/2/2 3/3/3
f 2//2 4//-3 3//-1
f -4 -3 -1
"""


def test_obj_reader_reads_vn_in_every_face_form():
    path = _write("normals_vn_forms.obj", OBJ_VN)
    p0, p1, p2, ng, vn = _flat_normals(_mesh_scene(path, "file"))
    assert vn is not None and vn.shape == (3, 9)
    by = {tuple(p1[i]) + tuple(p2[i]): vn[i] for i in range(3)}                                             # (the flattening follows the hierarchy's leaf order)
    assert np.array_equal(by[(2.0, 0.0, 0.0, 0.0, 2.0, 0.0)], np.array([0, 0, 1, 0.6, 0, 0.8, 0, 0.6, 0.8], f32))   # v/vt/vn
    assert np.array_equal(by[(2.0, 2.0, 1.0, 0.0, 2.0, 0.0)], np.array([0.6, 0, 0.8, 0, 0, 1, 0, 0.6, 0.8], f32))   # v//vn with negative indices
    assert not by[(2.0, 0.0, 0.0, 2.0, 2.0, 1.0)].any()                                                       # the face without vn stays flat


def test_default_stays_flat_for_a_file_with_vn():
    path = _write("normals_vn_forms.obj", OBJ_VN)
    assert _flat_normals(_mesh_scene(path, None))[4] is None


def test_flip_normal_and_handedness_act_on_the_file_normals():
    path = _write("normals_vn_forms.obj", OBJ_VN)
    a = _flat_normals(_mesh_scene(path, "file"))
    b = _flat_normals(_mesh_scene(path, "file", flip_normal=True))
    c = _flat_normals(_mesh_scene(path, "file", flip_hand=True))
    key = lambda r: {tuple(r[1][i]) + tuple(r[2][i]): i for i in range(3)}
    ka, kb = key(a), key(b)
    for k, i in ka.items():
        assert np.array_equal(b[4][kb[k]], -a[4][i]) and np.array_equal(b[3][kb[k]], -a[3][i])
    kc = {tuple(c[1][i] * (1, 1, -1)) + tuple(c[2][i] * (1, 1, -1)): i for i in range(3)}
    for k, i in ka.items():
        assert np.array_equal(c[4][kc[k]], a[4][i] * np.tile((1, 1, -1), 3).astype(f32))


def _cube():
    v = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = []
    for k, (a, b, c, d) in enumerate(quads):
        faces += [(a, b, c), (a, c, d)] if k % 2 == 0 else [(b, c, d), (b, d, a)]      # both diagonals occur
    return v, np.array(faces)


@pytest.mark.parametrize("angle", [100.0, 30.0])
def test_computed_normals_on_a_triangulated_cube(angle):
    v, f = _cube()
    path = scenes.write_obj(os.path.join(scenes.asset_dir(), "normals_cube.obj"), v, f)
    p0, p1, p2, ng, vn = _flat_normals(_mesh_scene(path, angle))
    assert vn is not None and len(vn) == 12
    pts = np.stack([p0, p1, p2], 1)
    for t in range(12):
        for k in range(3):
            want = pts[t, k] / np.sqrt(3.0) if angle == 100.0 else ng[t]
            assert np.abs(vn[t, 3 * k:3 * k + 3] - want).max() <= 1e-6
    # ... and the rule as tests/normals_ref.py states it gives the same
    ref = R.computed_normals(v, f, angle)
    key = lambda tri: tuple(sorted(map(tuple, np.asarray(tri, f32))))
    by_corner = {(key(v[list(face)]), tuple(v[face[k]])): ref[i, k] for i, face in enumerate(f) for k in range(3)}
    for t in range(12):
        for k in range(3):
            assert np.abs(vn[t, 3 * k:3 * k + 3] - by_corner[(key(pts[t]), tuple(pts[t, k]))]).max() <= 1e-6


def test_flattening_a_smooth_mesh_follows_the_triangle_order():
    v, f = R.icosphere(1)
    path = scenes.write_obj(os.path.join(scenes.asset_dir(), "normals_ico80.obj"), v.astype(f32), f)
    be = _mesh_scene(path, 180.0)
    p0, p1, p2, ng, vn = _flat_normals(be)
    assert vn.shape == (80, 9) and be.flatten().contents.n_triangles == 80
    # all 80 facets are within 180 degrees of each other: every corner gets its vertex's angle-weighted normal, which on the icosphere is radial
    for k, p in enumerate((p0, p1, p2)):
        assert np.abs(vn[:, 3 * k:3 * k + 3] - p / np.linalg.norm(p, axis=-1, keepdims=True)).max() <= 2e-3
    assert jp.check_vertex_normals(vn) == 80
