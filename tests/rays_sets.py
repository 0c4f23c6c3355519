"""Scenes and ray sets of the per-ray tests (tests/test_rays_host.py on the CPU, tests/test_gpu_occluded.py on the GPU), and their float64 results
(tests/rays_ref.py), computed once per (scene, set) and process.

Ray sets per scene (all fp32, as the library receives them):
  random     origins fill the scene's box, directions are normalised Gaussians (2 % with one zero component), tmin 0.001, half the far ends infinite and half
             uniform within the scene's size
  shadow     the rays FScene::Occluded forms, in fp32: P a camera ray's first hit (float64 reference, pushed nowhere), Q uniform on a primitive (half on the
             lights), dir = (Q - P) / |Q - P|, tmin 0.001, tmax |P - Q| - 0.001
             (all of them: the rays as a render makes them, for the checks that need no verdict)
  shadow_plain  the rays of `shadow` that leave P's surface and reach Q's at |cos| >= GRAZING.  The others are close calls by definition at that end: about a
             tenth of all shadow rays, so they stay out of the sets the 2 % cap is for
  shadow8    where 0.001 < 4 m (rays_ref.py) both ends of every shadow ray are close calls by definition -- P's own surface sits 0.001 before tmin, Q's
             0.001 behind tmax --: the rays of shadow_plain with tmin 8 m and tmax |P - Q| - 8 m, a decisive version
  near, far  rays of `random` with a decisive float64 nearest hit at t*: tmax = t* - 4 m' (the hit lies beyond the far end) and tmax = t* + 4 m' (it blocks)
  edges      groups of 64 that share a direction octant, mixed groups, groups with one odd lane, axis-parallel directions with zeros of both signs, origins
             exactly on the planes of the scene's walls; tmin 0, 0.001 and 0.05 S; tmax below tmin, 0, finite and infinite
Every set's size is odd or prime-ish, so the last wave is partial."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

import harness as H
import rays_ref as R

S_ = H.scenes
N_RANDOM, N_SHADOW, N_BRACKET, N_EDGES = 20011, 5003, 4999, 4099
N_TINY = 4099
TINY = ("one_triangle", "one_rectangle", "one_sphere", "one_disk", "two", "tri32", "tri33", "all_lights")
LARGE = "soup2000"
_tmp = None


def _tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="jp_rays_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def _soup(path, n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2.5, 2.5, (n, 1, 3))
    v = (c + rng.normal(0, 0.8, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    S_.write_obj(path, v, np.arange(3 * n).reshape(-1, 3))


def _tiny(hb, name):
    hb.camera((0, 0, 9), (0, 0, -1), (0, 1, 0), 55.0, 64, 64)
    hb.envlight((0.4, 0.5, 0.6))
    m = hb.mat_matte((0.6, 0.5, 0.4))
    if name in ("one_triangle", "tri32", "tri33"):
        n = {"one_triangle": 1, "tri32": 32, "tri33": 33}[name]
        path = os.path.join(_tmpdir(), name + ".obj")
        if n == 1:
            S_.write_obj(path, np.array([[-2.5, -2, 0.3], [2.5, -1.5, -0.4], [0.2, 2.5, 0.1]], np.float32), np.array([[0, 1, 2]]))
        else:
            _soup(path, n, n)
        hb.mesh(path, False, False, (0, 0, 0), 1.0, m, (3.0, 3.0, 3.0) if n == 1 else None)
    elif name == "one_rectangle":
        hb.rect(S_.AXIS_XY, -2, 2, -1.5, 2.5, 0.25, False, m, None)
    elif name == "one_sphere":
        hb.sphere((0.3, -0.2, 0.5), 1.7, m, None)
    elif name == "one_disk":
        hb.disk((0.2, 0.1, -0.3), (0.3, 0.5, 0.8), 2.2, m, None)
    elif name == "two":
        hb.rect(S_.AXIS_XY, -2, 2, -2, 2, 0.0, False, m, None)
        hb.sphere((0, 0, 2), 0.7, m, (4.0, 4.0, 4.0))
    elif name == "all_lights":
        hb.rect(S_.AXIS_XZ, -2, 2, -2, 2, 2.5, False, m, (5.0, 5.0, 5.0))
        hb.rect(S_.AXIS_YZ, -2, 2, -2, 2, -2.5, False, m, (2.0, 3.0, 4.0))
        hb.sphere((0.5, -0.5, 0.5), 0.8, m, (6.0, 5.0, 4.0))
        hb.disk((-0.5, -2.0, 0.0), (0.0, 1.0, 0.2), 1.5, m, (3.0, 3.0, 3.0))
    hb.preprocess()


def build(name, tree="host"):
    """-> (backend, flattened scene): the backend owns the arrays.  tree: "host" the host's SAH tree, "device" none (the upload builds one), "reference" /
    "certified" the reference's own tree (and the certified walk's tables)"""
    hb = S_.HostBackend(name)
    if tree == "device":
        hb.set_device_build(True)
    elif tree in ("reference", "certified"):
        hb.set_reference_tree(True, certified=(tree == "certified"))
    if name in TINY:
        _tiny(hb, name)
    elif name == LARGE:
        H.build_random_scene(hb, 32, 32, 11, n_tris=2000, tmpdir=_tmpdir())
    else:
        H.SCENES[name](hb, 48, 48)
    return hb, hb.flatten()


@functools.lru_cache(maxsize=None)
def shapes(name):
    hb, sp = build(name)
    return R.Shapes(sp.contents)


def _unit32(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _box(sh):
    """the scene's box, each axis at least half the diagonal long (a scene of one flat shape: a box with some depth)"""
    pad = np.maximum(0.0, 0.5 * sh.S - (sh.hi - sh.lo)) / 2
    return sh.lo - pad, sh.hi + pad


def _random(sh, n, rng):
    o = rng.uniform(*_box(sh), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    z = rng.random(n) < 0.02
    d[z, rng.integers(0, 3, n)[z]] = 0.0
    tmin = np.full(n, 0.001, np.float32)
    tmax = np.where(rng.random(n) < 0.5, np.inf, rng.random(n) * sh.S).astype(np.float32)
    return o, _unit32(d), tmin, tmax


def _camera_rays(sp, n, rng):
    cam = sp.contents.camera
    pxy = (rng.random((n, 2)) * [cam.res_x, cam.res_y]).astype(np.float32)
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    L = H.oracle_lib(); oh = H.oracle_scene(L, sp)
    L.jp_oracle_camera_rays(oh, n, H.ptr(pxy), H.ptr(o), H.ptr(d))
    L.jp_oracle_scene_free(oh)
    return o, d


def _points_on(sh, prims, rng):
    """one point per entry of prims, uniform on that primitive, float64"""
    q = np.zeros((len(prims), 3))
    u = rng.random((len(prims), 2))
    where = {k: {int(p): i for i, p in enumerate(a)} for k, a in ((0, sh.tri_prim), (1, sh.rect_prim), (2, sh.sph_prim), (3, sh.disk_prim))}
    for j, p in enumerate(prims):
        k = int(sh.kind[p]); i = where[k][int(p)]
        if k == R.TRIANGLE:
            v = sh.tri_v[i]; s = np.sqrt(u[j, 0])
            q[j] = (1 - s) * v[0] + s * (1 - u[j, 1]) * v[1] + s * u[j, 1] * v[2]
        elif k == R.RECTANGLE:
            v = sh.rect_v[i]
            q[j] = v[1] + u[j, 0] * (v[0] - v[1]) + u[j, 1] * (v[2] - v[1])
        elif k == R.SPHERE:
            z = 1 - 2 * u[j, 0]; r = np.sqrt(max(0.0, 1 - z * z)); ph = 2 * np.pi * u[j, 1]
            q[j] = sh.sph_c[i] + sh.sph_r[i] * np.array([r * np.cos(ph), r * np.sin(ph), z])
        else:
            n = sh.disk_n[i]
            a = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0]); a /= np.linalg.norm(a); b = np.cross(n, a)
            r = sh.disk_r[i] * np.sqrt(u[j, 0]); ph = 2 * np.pi * u[j, 1]
            q[j] = sh.disk_c[i] + r * np.cos(ph) * a + r * np.sin(ph) * b
    return q


def _normals_at(sh, prims, x):
    """unit normals of the primitives `prims` at their points x"""
    n = np.zeros((sh.n_prims, 3)); c = np.zeros((sh.n_prims, 3))
    for P in sh._polys:
        if P is not None:
            n[P["prim"]] = P["n"]
    n[sh.disk_prim] = sh.disk_n
    c[sh.sph_prim] = sh.sph_c
    curved = sh.kind[prims] == R.SPHERE
    out = n[prims]
    r = x - c[prims]
    out[curved] = (r / np.maximum(np.linalg.norm(r, axis=1, keepdims=True), 1e-300))[curved]
    return out


def _shadow(sh, sp, n, rng):
    """-> the rays of FScene::Occluded from surface points to points on primitives, fp32 throughout: (P, dir, |P - Q| in fp32, grazing), grazing: the ray
    leaves P's surface or reaches Q's at |cos| < GRAZING -- a close call by definition at that end, whatever lies in between"""
    o, d = _camera_rays(sp, 2 * n, rng)
    first = R.cast(sh, o, d, np.full(2 * n, 0.001), np.full(2 * n, np.inf))
    ok = np.nonzero(first["hit"])[0]
    if len(ok) == 0:
        return None
    pick = ok[rng.integers(0, len(ok), n)]
    P64 = o[pick].astype(np.float64) + first["t"][pick, None] * d[pick].astype(np.float64)
    P = P64.astype(np.float32)
    lights = np.nonzero(sh.light >= 0)[0]
    prims = rng.integers(0, sh.n_prims, n)
    if len(lights):
        prims[: n // 2] = lights[rng.integers(0, len(lights), n // 2)]
    Q64 = _points_on(sh, prims, rng)
    Q = Q64.astype(np.float32)
    v = Q - P                                                              # scene.h:36-47 in fp32: Normalize(target - p), Length(p - target)
    dist = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float32)
    keep = dist > np.float32(max(0.01, 32 * sh.m))                         # (Q on P's own spot: no ray)
    w = Q64 - P64; w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    cos_p = np.abs((_normals_at(sh, first["prim"][pick], P64) * w).sum(1)); cos_q = np.abs((_normals_at(sh, prims, Q64) * w).sum(1))
    grazing = (cos_p < R.GRAZING) | (cos_q < R.GRAZING)
    with np.errstate(invalid="ignore", divide="ignore"):
        dirs = (v / dist[:, None]).astype(np.float32)
    return P[keep], dirs[keep], dist[keep], grazing[keep]


def _edges(sh, rng):
    """the structure of test_gpu_flat_boxes._trace_rays on the scene's own box: 64 groups of 64 rays, and three more rays"""
    n = N_EDGES
    g = np.minimum(np.arange(n) // 64, 63)
    lo, hi = _box(sh)
    o = rng.uniform(lo + 0.01 * (hi - lo), hi - 0.01 * (hi - lo), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = _unit32(d)
    octant = np.array([[1 if (k >> a) & 1 else -1 for a in range(3)] for k in range(8)], np.float32)
    one = (g < 16) | ((g >= 32) & (g < 48))                               # groups 0-15: one octant each; 16-31: mixed; 32-47: one octant with one odd lane
    d[one] = np.abs(d[one]) * octant[g[one] % 8]
    for grp in range(32, 48):
        lane, axis = int(rng.integers(0, 64)), int(rng.integers(0, 3))
        d[grp * 64 + lane, axis] = -d[grp * 64 + lane, axis] if grp % 2 else np.float32(0.0) * (-1 if grp % 4 else 1)
    ax = (g >= 48) & (g < 56)                                             # 48-55: axis-parallel rays, zeros of both signs in the other components
    k = rng.integers(0, 3, n); sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    par = np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0); par[np.arange(n), k] = sgn
    d[ax] = par[ax].astype(np.float32)
    wall = g >= 56                                                       # 56-63: origins exactly on the planes of the walls (the coordinates the flat shapes' corners take)
    corners = np.concatenate([sh.rect_v.reshape(-1, 3), sh.tri_v.reshape(-1, 3)[:64], sh.lo[None], sh.hi[None]]).astype(np.float32)
    for i in np.nonzero(wall)[0]:
        a = int(rng.integers(0, 3)); o[i, a] = rng.choice(corners[:, a])
    # tmin: 0, 0.001 and 0.05 S by group; an origin on a wall sits on a primitive at t = 0, a close call for the first two: there only a few lanes take them
    tmin = np.array([0.0, 0.001, 0.05 * sh.S], np.float32)[g % 3]
    tmin[wall] = np.float32(0.05 * sh.S)
    few = wall & (g == 63) & (np.arange(n) % 64 < 32)
    tmin[few] = np.where(np.arange(n)[few] % 2 == 0, 0.0, 0.001).astype(np.float32)
    tmax = np.full(n, np.inf, np.float32)
    fin = g % 4 == 1
    tmax[fin] = rng.uniform(0.1 * sh.S, 0.7 * sh.S, n).astype(np.float32)[fin]     # every fourth group: a finite far end
    lane = np.arange(n) % 64
    tmax[(g % 16 == 3) & (lane % 7 == 0)] = np.float32(0.0005)                    # far ends below tmin (groups with tmin 0: just a short ray)
    tmax[(g % 16 == 7) & (lane % 5 == 0)] = np.float32(0.0)                       # tmax = 0
    tmax[(g % 16 == 11) & (lane % 6 == 0)] = tmin[(g % 16 == 11) & (lane % 6 == 0)] * np.float32(0.5)   # tmax < tmin
    return o, d, tmin, tmax


@functools.lru_cache(maxsize=None)
def ray_sets(name):
    """-> {set: (o, d, tmin, tmax)} for the scene, deterministic"""
    sh = shapes(name)
    hb, sp = build(name)
    rng = np.random.default_rng(abs(hash_name(name)))
    tiny = name in TINY
    out = {}
    n_rand = N_TINY if tiny else N_RANDOM
    out["random"] = _random(sh, n_rand, rng)
    s = _shadow(sh, sp, 1500 if tiny else N_SHADOW, rng)
    if s is not None:
        P, dirs, dist, gz = s
        if len(P) % 64 == 0:
            P, dirs, dist, gz = P[:-1], dirs[:-1], dist[:-1], gz[:-1]
        t0 = np.full(len(P), 0.001, np.float32); t1 = dist - np.float32(0.001)
        out["shadow"] = (P, dirs, t0, t1)                                 # every ray, in the order made
        if (~gz).any():
            out["shadow_plain"] = (P[~gz], dirs[~gz], t0[~gz], t1[~gz])   # ... without the ones that graze the surface at either end
        if 0.001 < 4 * sh.m and (~gz).any():
            m8 = np.float32(8 * sh.m)
            out["shadow8"] = (P[~gz], dirs[~gz], np.full(int((~gz).sum()), m8, np.float32), dist[~gz] - m8)
    # far-end brackets round decisive nearest hits
    nb = min(n_rand, 1499 if tiny else N_BRACKET)
    o, d, tmin, _ = (a[:nb] for a in out["random"])
    first = R.cast(sh, o, d, tmin, np.full(nb, np.inf))
    ok = first["hit"] & first["decisive"]
    if ok.any():
        ts = first["t"][ok]
        mp = 4 * sh.m * np.maximum(1.0, ts / sh.S)
        # (fp32 rounding of tmax moves it by t* 6e-8, a fraction of m')
        out["near"] = (o[ok], d[ok], tmin[ok], (ts - mp).astype(np.float32))
        out["far"] = (o[ok], d[ok], tmin[ok], (ts + mp).astype(np.float32))
    out["edges"] = _edges(sh, rng)
    return out


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) + 12345


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """the float64 result (rays_ref.cast) for one set of one scene"""
    o, d, tmin, tmax = ray_sets(name)[which]
    return R.cast(shapes(name), o, d, tmin, tmax)


def oracle_trace(sp, o, d, tmin, tmax):
    """jp_oracle_trace: the fp32 CPU oracle's closest hit -> (hit, t, prim)"""
    m = o.shape[0]
    L = H.oracle_lib(); oh = H.oracle_scene(L, sp)
    hit = np.zeros(m, np.int32); t = np.zeros(m, np.float32); prim = np.zeros(m, np.int32); nrm = np.zeros((m, 3), np.float32); pos = np.zeros((m, 3), np.float32)
    o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmin = np.ascontiguousarray(tmin, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
    L.jp_oracle_trace(oh, m, H.ptr(o), H.ptr(d), H.ptr(tmin), H.ptr(tmax), H.ptr(hit), H.ptr(t), H.ptr(prim), H.ptr(nrm), H.ptr(pos))
    L.jp_oracle_scene_free(oh)
    return hit, t, prim


def capped(name, which):
    """does the 2 % cap on non-decisive rays apply to this set?  Not to the sets made of close calls on purpose"""
    if which == "shadow":
        return False
    if which == "shadow_plain":
        return not (0.001 < 4 * shapes(name).m)
    return True


SCENES = ("cornell", "misc", "disks", "lights", LARGE, "bunny_small") + TINY
