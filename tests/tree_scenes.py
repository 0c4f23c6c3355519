"""Scenes for the structural tree tests (tests/test_tree_tables_host.py, tests/test_gpu_tree_tables.py): seeded mixes of all four shapes, as a JpScene over numpy
arrays (no hierarchy: the device builds it) or through HostBackend (the host builds it), and the primitive records of a JpScene in the caller's order.
TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

F = np.float32
TABLES = ("nodes", "prims", "meta", "wide", "q4", "flat")
INFO_FIELDS = ("n_prims", "n_nodes", "bvh_height", "n_wide", "wide_height", "n_q4", "q4_height")


class NumpyScene:
    """a JpScene without a hierarchy over arrays this object keeps alive: kinds (n,) shape type per primitive in creation order; centre (n, 3); size (n,)"""

    def __init__(self, kinds, centre, size, rng, planar=False, symmetric=False):
        kinds = np.asarray(kinds, np.int32); c = np.asarray(centre, F); s = np.asarray(size, F)
        n = kinds.size
        k = [np.flatnonzero(kinds == t) for t in range(4)]
        index = np.zeros(n, np.int32)
        for t in range(4):
            index[k[t]] = np.arange(k[t].size)
        a = {}
        # triangles: three points about the centre (symmetric: the box is centre -+ size exactly; planar: all in the plane z = centre.z)
        ct, st = c[k[0]], s[k[0]][:, None]
        if symmetric:
            d = np.array([[-1, -1, -1], [1, 1, -1], [-1, 1, 1]], F)[None] * st[:, None, :]
        else:
            d = (rng.uniform(-1, 1, (k[0].size, 3, 3)).astype(F)) * st[:, None, :]
        if planar:
            d[:, :, 2] = 0
        p = ct[:, None, :] + d
        a["tri_p0"], a["tri_p1"], a["tri_p2"] = (np.ascontiguousarray(p[:, j]) for j in range(3))
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(F)
        a["tri_n"] = np.ascontiguousarray(np.where(np.abs(nrm).sum(1, keepdims=True) > 0, nrm, F(1)))
        # rectangles in the plane z = centre.z: corners centre -+ (size, size / 2)
        cr, sr = c[k[1]], s[k[1]]
        ex = np.zeros((k[1].size, 3), F); ey = np.zeros((k[1].size, 3), F); ex[:, 0] = sr; ey[:, 1] = sr * F(0.5)
        a["rect_p0"], a["rect_p1"], a["rect_p2"], a["rect_p3"] = cr - ex - ey, cr + ex - ey, cr + ex + ey, cr - ex + ey
        a["rect_n"] = np.tile(np.array([0, 0, 1], F), (k[1].size, 1))
        a["sph_center"] = np.ascontiguousarray(c[k[2]]); a["sph_radius"] = np.ascontiguousarray(s[k[2]])
        a["disk_center"] = np.ascontiguousarray(c[k[3]]); a["disk_radius"] = np.ascontiguousarray(s[k[3]])
        dn = rng.normal(size=(k[3].size, 3)); dn /= np.maximum(np.linalg.norm(dn, axis=1, keepdims=True), 1e-9)
        a["disk_normal"] = np.ascontiguousarray(dn, F)
        a = {key: np.ascontiguousarray(v, F) for key, v in a.items()}
        a["prim_shape_type"] = kinds; a["prim_shape_index"] = index
        a["prim_material"] = (np.arange(n) % 2).astype(np.int32); a["prim_light"] = np.full(n, -1, np.int32)
        a["mat_type"] = np.zeros(2, np.int32); a["mat_params"] = np.full(2 * jp.JP_MAT_PARAM_STRIDE, 0.5, F)
        self.arrays = a
        sc = jp.JpScene()
        sc.camera.pos[:] = (0, 0, 9); sc.camera.front[:] = (0, 0, -1); sc.camera.right[:] = (0.5, 0, 0); sc.camera.up[:] = (0, 0.5, 0); sc.camera.res_x = sc.camera.res_y = 16
        sc.n_triangles, sc.n_rectangles, sc.n_spheres, sc.n_disks = (int(v.size) for v in k)
        sc.n_primitives = n; sc.n_materials = 2; sc.n_lights = 0; sc.world_radius = 1.0
        for key, v in a.items():
            setattr(sc, key, v.ctypes.data_as(type(getattr(sc, key))))
        self.scene = sc
        self.n = n

    def ptr(self):
        return C.pointer(self.scene)


def _as(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, (n,)).astype(dtype) if n else np.zeros(0, dtype)


def input_records(s):
    """the primitive records of a JpScene in the caller's order, laid out as the upload lays them out (csrc/jp_scene_host.h emit_prim):
    -> prims (n, 16) float32, meta (n, 4) int32"""
    if isinstance(s, C._Pointer):
        s = s.contents
    n = s.n_primitives
    t = _as(s.prim_shape_type, n, np.int32); i = _as(s.prim_shape_index, n, np.int32)
    v3 = lambda p, m: _as(p, 3 * m, F).reshape(-1, 3)
    g = np.zeros((n, 16), F)
    k = t == 0; j = i[k]
    for w, name in enumerate(("tri_p0", "tri_p1", "tri_p2", "tri_n")):
        g[k, 4 * w:4 * w + 3] = v3(getattr(s, name), s.n_triangles)[j]
    k = t == 1; j = i[k]
    for w, name in enumerate(("rect_p0", "rect_p1", "rect_p2", "rect_n")):
        g[k, 4 * w:4 * w + 3] = v3(getattr(s, name), s.n_rectangles)[j]
    p3 = v3(s.rect_p3, s.n_rectangles)[j]
    g[k, 3], g[k, 7], g[k, 11] = p3[:, 0], p3[:, 1], p3[:, 2]
    k = t == 2; j = i[k]
    g[k, 0:3] = v3(s.sph_center, s.n_spheres)[j]; g[k, 3] = _as(s.sph_radius, s.n_spheres, F)[j]
    k = t == 3; j = i[k]
    g[k, 0:3] = v3(s.disk_center, s.n_disks)[j]; g[k, 3] = _as(s.disk_radius, s.n_disks, F)[j]; g[k, 4:7] = v3(s.disk_normal, s.n_disks)[j]
    g.view(np.int32)[:, 15] = t
    meta = np.stack([np.arange(n, dtype=np.int32), _as(s.prim_material, n, np.int32), _as(s.prim_light, n, np.int32), t], axis=1)
    return g, meta


# ---- distributions of the device-build tests: n primitives of all four shapes (planar: the two flat ones, which alone have no extent across their plane) ----
def make(n, dist="uniform", seed=1):
    rng = np.random.default_rng([seed, n])
    kinds = rng.integers(0, 4, n)
    kinds[:min(n, 4)] = np.arange(4)[:min(n, 4)]                          # every shape, at every count from 4 up
    size = rng.uniform(0.005, 0.03, n)
    kw = {}
    if dist == "uniform":
        c = rng.uniform(-1, 1, (n, 3))
    elif dist == "coincident":                                           # one box centre, dyadic half extents: every Morton key equal
        c = np.tile(np.array([0.25, 0.5, -0.125]), (n, 1)); size = 2.0 ** -rng.integers(4, 9, n); kw["symmetric"] = True
    elif dist == "planar":                                               # zero extent along z
        kinds = kinds % 2; c = rng.uniform(-1, 1, (n, 3)); c[:, 2] = 0.375; kw["planar"] = True
    elif dist == "clusters":                                             # two tight clusters far apart: the keys differ in their top bits only
        c = np.where(rng.integers(0, 2, (n, 1)) == 0, -1000.0, 1000.0) + rng.uniform(-1e-4, 1e-4, (n, 3)); c[0] = -1000.0; c[1] = 1000.0; size = np.full(n, 1e-4)
    elif dist == "cell":                                                 # a dense grid inside 2^-13 of the scene's extent (two far primitives span it): only the low key bytes differ
        m = int(np.ceil((n - 2) ** (1 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n - 2]
        c = np.concatenate([[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], 0.1 + g * (2.0 ** -12 / m)]); size = np.concatenate([[0.01, 0.01], np.full(n - 2, 2.0 ** -14 / m)])
    else:
        raise ValueError(dist)
    return NumpyScene(kinds, c, size, rng, **kw)


# ---- a host-built scene of exactly n primitives, all four shapes (HostBackend: the host's SAH builder makes the tree) ----------------------------------
def host_backend(n, tmpdir, seed=3):
    rng = np.random.default_rng([seed, n])
    be = scenes.HostBackend("tree_%d" % n)
    be.set_device_build(False)
    be.camera((0, 0, 9), (0, 0, -1), (0, 1, 0), 55.0, 16, 16)
    be.envlight((0.2, 0.2, 0.2))
    m = be.mat_matte((0.5, 0.5, 0.5))
    n_tri = n - 3 * (n // 8)                                              # most are triangles (one mesh), an eighth each spheres, disks, rectangles
    c = rng.uniform(-2, 2, (n_tri, 1, 3)); v = (c + rng.normal(0, 0.1, (n_tri, 3, 3))).reshape(-1, 3).astype(F)
    path = os.path.join(str(tmpdir), "tree_%d.obj" % n)
    scenes.write_obj(path, v, np.arange(3 * n_tri).reshape(-1, 3))
    be.mesh(path, False, False, (0, 0, 0), 1.0, m, None)
    for _ in range(n // 8):
        be.sphere(tuple(rng.uniform(-2, 2, 3)), float(rng.uniform(0.02, 0.2)), m, None)
        be.disk(tuple(rng.uniform(-2, 2, 3)), tuple(rng.normal(size=3)), float(rng.uniform(0.02, 0.2)), m, None)
        a, b = rng.uniform(-2, 1.8, 2)
        be.rect(int(rng.integers(0, 3)), float(a), float(a + rng.uniform(0.02, 0.2)), float(b), float(b + rng.uniform(0.02, 0.2)), float(rng.uniform(-2, 2)), False, m, None)
    be.preprocess()
    assert be.num_primitives() == n
    return be


def host_tables(scene_ptr, options=None, light_mode="all"):
    """-> (tabs of jp_copy_upload_table, info dict, JpUploadInfo)"""
    i = jp.describe_upload(scene_ptr, options, light_mode)
    tabs = {k: jp.copy_upload_table(scene_ptr, k, options, light_mode) for k in TABLES}
    return tabs, {k: int(getattr(i, k)) for k in INFO_FIELDS}, i


def device_tables(ctx):
    """-> (tabs of jp_read_scene_table, info dict)"""
    i = ctx.tree_info()
    return {k: ctx.read_table(k) for k in TABLES}, {k: int(getattr(i, k)) for k in INFO_FIELDS}


def fnv1a(b):
    """64-bit FNV-1a of a uint8 array"""
    h = 1469598103934665603
    for v in b.tobytes():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
