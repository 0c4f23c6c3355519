"""The feature oracle (oracle/pt_features.cc, INTEGRATION.md "Feature oracle") checked on the CPU alone: it reduces to jp_oracle_render bit for bit wherever a
feature cannot act, its estimators meet the closed forms the GPU tests of the features use, NEE and MIS agree in the mean, the film does not depend on the
thread count, and for every cell of the GPU matrix (tests/test_gpu_oracle_features.py imports SCENES / FAMILIES / CELLS from here) at most 1 % of the
pixels are undecided.  No GPU: jp_build_light_table, jp_build_environment_table and the scene flattener are pure host code."""
import ctypes as C
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import harness as H
import mis_ref as M
import normals_ref as R

f32 = np.float32
SPP, DEPTH, SEED = 16, 6, 4242                                     # every cell: 16 spp, depth 6 (Russian roulette from bounce 3 takes part), the counter sampler


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the scenes of the matrix ---------------------------------------------------------------------------------------------------------------------
# One room ("zoo"), in variants that differ in what the upload's plan makes of them (tests/test_gpu_oracle_features.py, docstring):
#   zoo           ~100 primitives, 8 lit lights: tables and primitive records in LDS; JP_LIGHTS_ALL has more than 4 shadow planes, so its rows are unstaged
#   zoo_few       the same room with 3 lit lights and without the small icosphere: the staged rows of JP_LIGHTS_ALL (three staging planes next to the records in LDS)
#   zoo_bulk      + a 320-triangle icosphere: the primitive records no longer fit LDS
#   zoo_bulk_few  that with 3 lit lights: staged, the records in global memory
#   zoo_mats      + 270 unused materials: the tables no longer fit LDS
#   cornell, cornell_null  the Cornell box of the base tests (flat shapes, matte and metal, one area light; with a null-material rectangle): the lean instances of k_shade
# Contents (between them): area lights on a rectangle, a triangle pair, a disk and a sphere (whose own matte surface holds shading points with
# len2(p - c) <= r^2: the "inside" branch of its sampler and the unweighed case of MIS); a point, a directional, a constant environment and a black light; matte,
# mirror, plastic, metal, glass; a null-material rectangle below the triangle light (the carried MIS record); a smooth 80-triangle icosphere with a point light
# below the geometric horizon of many of its faces (the guard); image and checker textures on rectangles, triangles, disks and spheres; a normal-mapped wall.
#   zoo_one_sided  (host test of NEE against MIS only) the rectangle light replaced by a disk: FRectangle turns its normal toward every ray, so a rectangle light
#             emits at a hit from behind while sample_li never returns radiance from there; MIS counts that emission ("One-sided lights")
#             and NEE does not.  In the other variants the ceiling 0.02 above the rectangle light receives it, which the matrix pins and which makes the MIS films
#             about 2 % brighter on the walls next to the lamp.  It also has no null-material rectangle: FScene::Occluded stops at a primitive whatever its material,
#             so next-event estimation never reaches the triangle light through it, while the BSDF sample's ray passes and MIS counts what it finds.
SIZES = {"zoo": (32, 24), "zoo_few": (30, 22), "zoo_bulk": (48, 32), "zoo_bulk_few": (32, 24), "zoo_mats": (32, 24), "zoo_one_sided": (32, 24), "cornell": (32, 24), "cornell_null": (32, 24)}   # 30 x 22 x 16 samples: no multiple of the 256-thread block
ICO_CENTER, ICO_RADIUS = (-0.3, 3.4, -4.6), 0.9
BULK_CENTER, BULK_RADIUS = (2.4, 4.4, -6.2), 0.7


def _image(seed, h=8, w=16):
    """a coarse power-of-two image with strong texel-to-texel contrast"""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 5, (h, w, 3)) * 51).astype(np.uint8)


def _image_mip(seed, h, w):
    """an image large enough to have levels, with texel-to-texel contrast at every level of its pyramid: the sum of one random block pattern per level, the
    pattern of level k constant over 2^k x 2^k texels (so the 2 x 2 averages leave it whole down to level k)"""
    rng = np.random.default_rng(seed)
    n = int(np.log2(max(h, w))) + 1
    acc = np.zeros((h, w, 3))
    for k in range(n):
        b = rng.integers(0, 256, (max(1, h >> k), max(1, w >> k), 3)).astype(np.float64)
        acc += np.repeat(np.repeat(b, 1 << k, 0), 1 << k, 1)[:h, :w]
    return np.clip(np.round(acc / n * 1.6 - 76.0), 0, 255).astype(np.uint8)


def _nmap_image():
    rng = np.random.default_rng(31)
    img = np.full((8, 8, 3), 128, np.uint8)
    img[..., 0] = rng.integers(60, 200, (8, 8)); img[..., 1] = rng.integers(60, 200, (8, 8)); img[..., 2] = 255
    return img


def env_map_rgb():
    """16 x 8, coarse: two values in blocks and one bright texel in the row next to the north pole"""
    rgb = np.full((8, 16, 3), 1.0, f32)
    rgb[:, 8:] = (0.5, 0.75, 1.5)
    rgb[1, 3] = (300.0, 260.0, 180.0)
    return rgb


def _asset(name, verts, faces, uvs=None):
    return scenes.write_obj(os.path.join(scenes.asset_dir(), "oracle_features_%s.obj" % name), np.asarray(verts, f32), np.asarray(faces), uvs)


def _quad_asset(name, p, uv=True):
    return _asset(name, p, [(0, 1, 2), (0, 2, 3)], np.array([(0, 0), (1, 0), (1, 1), (0, 1)], f32) if uv else None)


def _ico_asset(sub, center, radius):
    v, f = R.icosphere(sub, radius, R.generic_rotation())
    return _asset("ico%d" % sub, v + np.asarray(center), f)


# The mip / proc variant of the room (build_zoo(mip=..., proc=...)); the values below were chosen on the CPU until test_new_groups_reach_every_branch held in
# every new group, and are conditions on the inputs, not measurements of the device:
#   MIP_SIZES          the rectangle image (floor) and the triangle image (back wall); the sphere and disk images keep 16 x 8 and stay JP_MIP_OFF -- a trilinear
#                      lookup on their uv is undecided always, and the cap on undecided pixels is 1 %
#   MIP_FOOTPRINT, MIP_SPREAD   JpTextureMipmaps.footprint_scale and bounce_spread of every mip family
#   proc_records()     one record per checker texture of the proc variant (which has three more of them than the plain room: the right wall, the icosphere, the emitters' matte)
MIP_SIZES = {"floor": (32, 64), "back": (4, 4)}                   # (h, w)
MIP_FOOTPRINT, MIP_SPREAD = 2.5, 0.125


def _rot_scale(s, t=(0.0, 0.0, 0.0)):
    """a non-identity 3 x 4 map: a generic rotation times s, and a translation"""
    R = R_generic()
    return tuple(np.concatenate([s * R, np.asarray(t, np.float64)[:, None]], 1).reshape(-1))


def R_generic():
    return np.asarray(R.generic_rotation(), np.float64)[:3, :3]


def proc_records(antialias=0):
    """name of the checker texture -> its JpProcedural.  Every kind; SPACE_UV on the triangle ceiling; SPACE_WORLD on the mirror sphere; the noise record with
    antialiasing off (all of them with antialias=-1); a non-identity map on the left wall; three CHECKER_AA records whose scales put the footprints of the room
    (widths of 0.2 .. 5) below the plain-checker threshold, inside the filtered range and across the 0.5 threshold"""
    P = jp.procedural
    d = lambda s: (s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0)
    return {
        "left": P(jp.JP_PROC_TURBULENCE, jp.JP_PROC_SPACE_WORLD, _rot_scale(0.1, (0.4, -1.3, 2.2)), octaves=3, gain=0.6, antialias=antialias),
        "ceil": P(jp.JP_PROC_FBM, jp.JP_PROC_SPACE_UV, (0.08, 0, 0, 0.45, 0, 0.07, 0, 0.55, 0, 0, 0.05, 0), octaves=2, antialias=antialias),
        "mirror": P(jp.JP_PROC_MARBLE, jp.JP_PROC_SPACE_WORLD, d(0.1), octaves=3, variation=2.0, antialias=antialias),
        "disk_b": P(jp.JP_PROC_NOISE, jp.JP_PROC_SPACE_WORLD, d(3.0), antialias=-1),
        "right": P(jp.JP_PROC_CHECKER_AA, jp.JP_PROC_SPACE_WORLD, d(1.0), antialias=antialias),
        "white": P(jp.JP_PROC_CHECKER_AA, jp.JP_PROC_SPACE_WORLD, (0.01, 0, 0, 0.003, 0, 0.01, 0, -0.034, 0, 0, 0.01, 0.5), antialias=antialias),
        "light": P(jp.JP_PROC_CHECKER_AA, jp.JP_PROC_SPACE_WORLD, d(1200.0), antialias=antialias),
    }


def build_zoo(variant, textured=False, nmap=False, records=False, reference_tree=True, mip=False, proc=False):
    W, Hh = SIZES[variant]
    be = scenes.HostBackend("oracle_features_" + variant)
    if reference_tree:
        be.set_reference_tree(True)                                # both sides walk the reference's tree: hits in a triangle's acceptance fringe agree
    if variant.startswith("cornell"):
        assert not (textured or nmap or records)
        null = (lambda b, m: b.rect(scenes.AXIS_XY, 150, 400, 100, 400, -100, False, -1, None)) if variant == "cornell_null" else None
        return scenes.build_cornell(be, W, Hh, lambert_only=False, extras=null)
    be.camera((0.0, 3.0, 10.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 45.0, W, Hh)
    few = variant in ("zoo_few", "zoo_bulk_few")
    be.envlight((0.05, 0.06, 0.1))                                 # light 0: the constant environment, or the tint of the map
    if not few:
        be.pointlight((-2.2, 2.2, -4.4), (5.0, 5.0, 4.0))          # beside the icosphere and below the horizon of its upper faces
        be.dirlight((0.3, -1.0, -0.4), (0.5, 0.45, 0.4))
    be.pointlight((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))                # a black light: pmf 0, never sampled, its draws consumed in JP_LIGHTS_ALL
    rec = jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_MIRROR, jp.JP_FILTER_BILINEAR, (2.0, 1.5), (0.25, 0.0)) if records else None
    be.zoo_tex = {}                                                # name -> texture index, for the mipmap modes and the procedural records

    def named(name, make):
        def f():
            be.zoo_tex[name] = make()
            return be.zoo_tex[name]
        return f
    img = lambda seed, sampling=None, name=None: named(name, lambda: be.texture_image(_image_mip(seed, *MIP_SIZES[name]) if (mip and name in MIP_SIZES) else _image(seed), sampling=sampling))
    chk = lambda a, b, name=None: named(name, lambda: be.texture_checker(a, b))

    def matte(rgb, tex=None):
        return be.mat_matte(tex=tex()) if (textured and tex) else be.mat_matte(rgb)
    m_floor = matte((0.7, 0.7, 0.65), img(1, rec, "floor"))                                       # rectangle, image (under a sampling record when asked)
    m_left = matte((0.63, 0.065, 0.05), chk((0.63, 0.065, 0.05), (0.2, 0.3, 0.6), "left")) # rectangle, checker; the normal-mapped wall
    m_right = matte((0.14, 0.45, 0.091), chk((0.14, 0.45, 0.091), (0.6, 0.6, 0.2), "right") if proc else None)
    m_back = matte((0.7, 0.7, 0.7), img(2, None, "back"))                                   # triangles, image
    m_ceil = matte((0.75, 0.75, 0.75), chk((0.8, 0.8, 0.8), (0.3, 0.5, 0.3), "ceil")) # triangles, checker
    m_white = matte((0.73, 0.71, 0.68), chk((0.73, 0.71, 0.68), (0.3, 0.4, 0.7), "white") if proc else None)
    m_light = matte((0.65, 0.65, 0.65), chk((0.65, 0.65, 0.65), (0.2, 0.2, 0.2), "light") if proc else None)
    m_mirror = be.mat_mirror(tex=chk((0.9, 0.9, 0.9), (0.9, 0.5, 0.3), "mirror")()) if textured else be.mat_mirror((0.9, 0.9, 0.9))          # sphere, checker
    ks = (0.3, 0.25, 0.2)
    m_plastic = be.mat_plastic(None, ks, 0.3, True, tex=img(3, None, "sphere")()) if textured else be.mat_plastic((0.35, 0.12, 0.48), ks, 0.3, True)   # sphere, image
    m_metal = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.3, False)
    m_glass = be.mat_glass(1.5, (0.98, 0.98, 0.98), (0.96, 0.98, 0.96))
    m_disk_a = matte((0.6, 0.55, 0.3), img(4, None, "disk_a"))                                # disk, image
    m_disk_b = matte((0.3, 0.55, 0.6), chk((0.3, 0.55, 0.6), (0.7, 0.2, 0.2), "disk_b"))   # disk, checker
    if variant == "zoo_mats":
        for k in range(270):
            be.mat_matte((0.5, 0.5, 0.5))                          # 270 x 64 bytes of material records: the shading tables exceed their 16 KB of LDS
    if nmap:
        be.mat_set_normal_map(m_left, be.normal_map(_nmap_image(), sampling=jp.tex_sampler(jp.JP_WRAP_REPEAT, jp.JP_WRAP_REPEAT, jp.JP_FILTER_BILINEAR, (3.0, 2.0)) if records else None), 0.8)
    be.rect(scenes.AXIS_XZ, -4.0, 4.0, -8.0, 1.0, 0.0, False, m_floor)
    be.rect(scenes.AXIS_YZ, 0.0, 6.0, -8.0, 1.0, -4.0, False, m_left)
    be.rect(scenes.AXIS_YZ, 0.0, 6.0, -8.0, 1.0, 4.0, False, m_right)
    be.mesh(_quad_asset("back", [(-4, 0, -8), (4, 0, -8), (4, 6, -8), (-4, 6, -8)]), False, False, mat=m_back)
    be.mesh(_quad_asset("ceiling", [(-4, 6, -8), (4, 6, -8), (4, 6, 1), (-4, 6, 1)]), False, False, mat=m_ceil)
    # area lights: rectangle and sphere always; the triangle pair and the disk unless `few`
    if variant == "zoo_one_sided":
        be.disk((-2.5, 5.98, -4.5), (0.0, -1.0, 0.0), 0.56, m_light, (14.0, 12.0, 9.0))
    else:
        be.rect(scenes.AXIS_XZ, -3.0, -2.0, -5.0, -4.0, 5.98, True, m_light, (14.0, 12.0, 9.0))
    be.sphere((-2.8, 0.8, -5.6), 0.45, m_light, (9.0, 8.0, 12.0))
    if not few:
        be.mesh(_quad_asset("lamp", [(1.0, 5.97, -4.0), (2.2, 5.97, -4.0), (2.2, 5.97, -3.0), (1.0, 5.97, -3.0)], uv=False), False, False, mat=m_light, radiance=(15.0, 11.0, 6.0))
        be.disk((3.3, 3.0, -6.0), scenes._normalize((-1.0, 0.0, 0.3)), 0.5, m_light, (10.0, 12.0, 8.0))
        if variant != "zoo_one_sided":
            be.rect(scenes.AXIS_XZ, 0.5, 2.7, -4.5, -2.5, 5.5, False, -1, None)   # null material below the triangle light: paths pass through, same bounce
    be.sphere((-1.6, 1.0, -4.0), 1.0, m_mirror)
    be.sphere((1.2, 0.9, -2.4), 0.9, m_glass)
    be.sphere((2.7, 0.7, -5.0), 0.7, m_plastic)
    be.disk((-3.0, 2.6, -6.6), scenes._normalize((0.6, 0.3, 0.7)), 0.9, m_metal)
    be.disk((0.0, 0.02, -5.6), (0.0, 1.0, 0.0), 0.8, m_disk_a)
    be.disk((3.4, 1.6, -2.6), scenes._normalize((-1.0, 0.2, 0.3)), 0.6, m_disk_b)
    if variant != "zoo_few":
        be.mesh(_ico_asset(1, ICO_CENTER, ICO_RADIUS), False, False, mat=m_white)
    if variant.startswith("zoo_bulk"):
        be.mesh(_ico_asset(2, BULK_CENTER, BULK_RADIUS), False, False, mat=m_metal)
    be.preprocess()
    return be


def zoo_vertex_normals(s):
    """radial normals on the triangles of the icospheres, every other triangle flat"""
    n = s.n_triangles
    P = [np.ctypeslib.as_array(p, (3 * n,)).reshape(n, 3).astype(np.float64) for p in (s.tri_p0, s.tri_p1, s.tri_p2)]
    vn = np.zeros((n, 9), f32)
    for c, r in ((ICO_CENTER, ICO_RADIUS), (BULK_CENTER, BULK_RADIUS)):
        on = np.all([np.abs(np.linalg.norm(p - np.asarray(c), axis=1) - r) < 1e-3 for p in P], 0)
        for k, p in enumerate(P):
            d = p[on] - np.asarray(c)
            vn[on, 3 * k:3 * k + 3] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return vn


# ---- feature sets -------------------------------------------------------------------------------------------------------------------------------------
# name -> (light sampling, map, estimator, textured, vertex normals): every combination the README claims -- light sampling all / power, map or none, NEE / MIS,
# textured or not, each with and without vertex normals (the map and MIS need the light table, so 2 + 2 * 2 * 2 = 10 families, twice)
def _families():
    out = {}
    for smooth in (False, True):
        for tex in (False, True):
            for mode, env, est in (("all", False, "nee"), ("power", False, "nee"), ("power", True, "nee"), ("power", False, "mis"), ("power", True, "mis")):
                name = ("smooth_" if smooth else "") + {("all", False, "nee"): "all", ("power", False, "nee"): "pick", ("power", True, "nee"): "env",
                                                          ("power", False, "mis"): "mis", ("power", True, "mis"): "mis_env"}[(mode, env, est)] + ("_tex" if tex else "")
                out[name] = dict(mode=mode, env=env, est=est, tex=tex, smooth=smooth, nmap=False, records=False, lens=False, film=False, mip=False, proc=False)
    # normal maps, sampling records, the lens and the film state on top of two of them
    for base in ("pick_tex", "smooth_mis_env_tex"):
        out[base + "_extras"] = dict(out[base], nmap=True, records=True, lens=True, film=True)
    # the ray cone (INTEGRATION.md sections 18, 19).  mip: JP_MIP_TRILINEAR on the rectangle and triangle images (k_texel_m).  proc: the records of proc_records()
    # on the checker textures (k_texel_p) -- "aa": antialiased (the cone array exists with or without pyramids), "off": every record with antialias off (k_texel_p
    # without a cone array).  The floor image is under a sampling record in the mip families (an active record's scale enters rho; the back wall takes the identity record).
    out["all_tex_mip"] = dict(out["all_tex"], mip=True, records=True)
    out["mis_env_tex_mip"] = dict(out["mis_env_tex"], mip=True, records=True)
    out["pick_tex_proc"] = dict(out["pick_tex"], proc="aa", spread=0.2)   # no pyramid: the mipmap state (all modes OFF) still carries the cone's bounce_spread
    out["pick_tex_proc_off"] = dict(out["pick_tex"], proc="off")
    out["mis_env_tex_mip_proc"] = dict(out["mis_env_tex"], mip=True, records=True, proc="aa")
    out["smooth_mis_env_tex_mip_proc_extras"] = dict(out["smooth_mis_env_tex_extras"], mip=True, proc="aa")
    return out


FAMILIES = _families()
LENS = dict(radius=0.15, focus_distance=13.0, blades=5, rotation_deg=12.0)
FILM = dict(hdr=1, sample_clamp=4.0)

_scene_cache = {}


def scene_of(variant, fam, reference_tree=True):
    key = (variant, fam["tex"], fam["nmap"], fam["records"], reference_tree, fam["mip"], bool(fam["proc"]))
    if key not in _scene_cache:
        _scene_cache[key] = build_zoo(variant, fam["tex"], fam["nmap"], fam["records"], reference_tree, fam["mip"], bool(fam["proc"]))
    return _scene_cache[key]


def zoo_mipmaps(be, footprint_scale=None, bounce_spread=None, on=("floor", "back")):
    """JP_MIP_TRILINEAR on the rectangle and the triangle image; the sphere and disk images stay JP_MIP_OFF (mixed modes)"""
    n = be.flatten_textures().contents.n_textures
    modes = [jp.JP_MIP_OFF] * n
    for name in on:
        modes[be.zoo_tex[name]] = jp.JP_MIP_TRILINEAR
    return jp.texture_mipmaps(modes, MIP_FOOTPRINT if footprint_scale is None else footprint_scale, MIP_SPREAD if bounce_spread is None else bounce_spread)


def zoo_procedurals(be, mode):
    t = be.flatten_textures().contents
    recs = [None] * t.n_textures
    for name, r in proc_records(-1 if mode == "off" else 0).items():
        assert t.tex_type[be.zoo_tex[name]] == jp.JP_TEXTURE_CHECKER
        recs[be.zoo_tex[name]] = r
    return jp.texture_procedurals(recs)


def state_of(variant, fam, reference_tree=True):
    """everything a Context needs for the family on the variant, and the same as the oracle's feature struct"""
    be = scene_of(variant, fam, reference_tree)
    sp = be.flatten()
    st = dict(be=be, sp=sp, mode=fam["mode"], est=fam["est"], rgb=env_map_rgb() if fam["env"] else None,
              textures=be.flatten_textures() if fam["tex"] else None,
              vn=zoo_vertex_normals(sp.contents) if fam["smooth"] else None,
              nmaps=be.flatten_normal_maps() if fam["nmap"] else None, sampling=be.flatten_texture_sampling() if fam["records"] else None,
              lens=jp.lens(**LENS) if fam["lens"] else None, film=jp.film(**FILM) if fam["film"] else None,
              mipmaps=zoo_mipmaps(be) if fam["mip"] else (zoo_mipmaps(be, 0.0, fam["spread"], on=()) if fam.get("spread") else None), procedurals=zoo_procedurals(be, fam["proc"]) if fam["proc"] else None)
    st["features"] = H.oracle_features(sp, st["mode"], st["rgb"], "y", 0, st["est"], None if st["vn"] is None else jp.vertex_normals(st["vn"]), st["textures"], st["sampling"],
                                       st["nmaps"], st["lens"], st["film"], mipmaps=st["mipmaps"], procedurals=st["procedurals"])
    W, Hh = SIZES[variant]
    st["params"] = jp.render_params(W, Hh, SPP, DEPTH, SEED)
    return st


_oracle_cache = {}


def oracle_of(variant, family, reference_tree=True):
    """(state, film, counters, undecided) of the oracle for one (scene, feature set): computed once, shared by every row and by both test files, never changed"""
    key = (variant, family, reference_tree)
    if key not in _oracle_cache:
        st = state_of(variant, FAMILIES[family], reference_tree)
        st["stats"] = H.JpOracleBranchStats()
        film, cnt, und = H.oracle_render_features(st["sp"], st["params"], st["features"], 8, stats=st["stats"])
        film.setflags(write=False); und.setflags(write=False)
        _oracle_cache[key] = (st, film, cnt, und)
    return _oracle_cache[key]


# ---- kernel rows ----------------------------------------------------------------------------------------------------------------------------------------
# (variant, family, options): the options reach the instance, the variant the row of the selector (tests/test_gpu_oracle_features.py lists them)
def _cells():
    cells = []
    for name, fam in FAMILIES.items():
        if fam["mip"] or fam["proc"]:
            continue                                              # the cone families: below
        if name.endswith("_extras") or fam["smooth"]:
            variants = ["zoo"]                                    # a scene with a shading normal of its own is planned onto the one row the smooth kernels have
        elif fam["mode"] == "all":
            variants = ["zoo", "zoo_few", "zoo_bulk", "zoo_bulk_few", "zoo_mats"]
        else:
            variants = ["zoo", "zoo_bulk", "zoo_mats"]            # one shadow plane: a scene whose tables fit LDS is always staged
        for v in variants:
            for sort in (1, -1):
                cells.append((v, name, dict(shade_sort=sort)))
    # the generic instance against the plan's choice, and one lane against three (a scene with a null-material primitive renders in one lane whatever is asked, so
    # these run in the room without one), on one family of each group
    for name in ("all", "mis_env_tex", "smooth_pick"):
        cells.append(("zoo", name, dict(shade_sort=1, generic=True)))
        cells.append(("zoo_bulk_few", name, dict(shade_sort=1, lanes=1)))
        cells.append(("zoo_bulk_few", name, dict(shade_sort=1, lanes=3)))
    # the cone families (k_texel_m, k_texel_p): every selector row a scene of theirs can reach, both orders; one mip and one procedural family through six batches
    # of the same slots, the last one short (max_slots = 3 W H: 3 of the 16 samples a pixel per batch), in one lane and in three; the generic instance on one
    for name, fam in FAMILIES.items():
        if fam["mip"] or fam["proc"]:
            for v in (["zoo"] if fam["smooth"] else ["zoo", "zoo_bulk", "zoo_mats"]):
                for sort in (1, -1):
                    cells.append((v, name, dict(shade_sort=sort)))
    for name in ("mis_env_tex_mip", "pick_tex_proc"):
        for lanes in (1, 3):
            cells.append(("zoo_bulk_few", name, dict(shade_sort=1, lanes=lanes, max_slots="3wh")))
    cells.append(("zoo", "mis_env_tex_mip_proc", dict(shade_sort=1, generic=True)))
    # the lean instances of k_shade and the generic one on the same scene
    cells += [("cornell", "all", dict(shade_sort=1)), ("cornell", "all", dict(shade_sort=-1)), ("cornell", "all", dict(shade_sort=1, generic=True)), ("cornell_null", "all", dict(shade_sort=1))]
    return cells


# the row of the kernel selector (jp_render.h shade_choice) each variant reaches: (tables in LDS, primitive records in
# LDS, next-event entries staged) in JP_LIGHTS_ALL and in JP_LIGHTS_POWER_ONE; a scene with smooth triangles or normal maps: (0, 0, 0) whatever its size
ROWS = {"zoo": ((1, 1, 0), (1, 1, 1)), "zoo_few": ((1, 1, 1), (1, 1, 1)), "zoo_bulk": ((1, 0, 0), (1, 0, 1)), "zoo_bulk_few": ((1, 0, 1), (1, 0, 1)), "zoo_mats": ((0, 0, 0), (0, 0, 0)),
        "cornell": ((1, 1, 1), (1, 1, 1)), "cornell_null": ((1, 1, 1), (1, 1, 1))}


def expected_row(variant, fam):
    if fam["smooth"] or fam["nmap"]:
        return (0, 0, 0)
    return ROWS[variant][0 if fam["mode"] == "all" else 1]


CELLS = _cells()


def cell_id(c):
    v, f, o = c
    return "%s-%s-%s" % (v, f, "_".join("%s%s" % (k, "" if o[k] is True else o[k]) for k in sorted(o)))


CONE_GROUPS = sorted({(v, f) for v, f, _ in CELLS if FAMILIES[f]["mip"] or FAMILIES[f]["proc"]})


GROUPS = sorted({(v, f) for v, f, _ in CELLS})


# ---- 1. reductions, bit for bit, against jp_oracle_render --------------------------------------------------------------------------------------------
def _base(sp, rp, **kw):
    return H.oracle_render(sp, rp, 4, **kw)


def _feat(sp, rp, **kw):
    return H.oracle_render_features(sp, rp, H.oracle_features(sp, **kw) if kw else None, 4)


def _counts(c):
    return (c.closest_rays, c.closest_hits, c.shadow_rays, c.shadow_occluded)


@pytest.mark.parametrize("name", ["cornell", "misc", "lights", "disks", "bunny_small"])
def test_no_features_is_the_base_oracle(name):
    W, Hh = 40, 30
    be = H.SCENES[name](scenes.HostBackend(name), W, Hh)             # (kept alive: the flattened arrays are the backend's)
    sp = be.flatten()
    rp = jp.render_params(W, Hh, 8, DEPTH, 99)
    a, ca = _base(sp, rp)
    b, cb, und = _feat(sp, rp)
    assert a.mean() > 0.02 and same(a, b) and _counts(ca) == _counts(cb) and cb.samples == W * Hh * 8 and not und.any()
    # ... also with every struct present and inert: all-flat normals, no texture on any material, lens radius 0, film all zero, NEE, JP_LIGHTS_ALL
    s = sp.contents
    inert = dict(light_mode="all", estimator="nee", normals=jp.vertex_normals(np.zeros((s.n_triangles, 9), f32)),
                 textures=jp.textures([jp.JP_TEXTURE_SOLID], [(0.3, 0.3, 0.3, 0, 0, 0)], np.full(s.n_materials, -1), s.n_triangles), lens=jp.lens(0.0), film=jp.film(0, 0.0))
    c, cc, und = _feat(sp, rp, **inert)
    assert same(a, c) and _counts(ca) == _counts(cc) and not und.any()
    # Whitted and the debug integrator pass through
    for integ in (jp.JP_INTEGRATOR_WHITTED, jp.JP_INTEGRATOR_DEBUG_NORMAL):
        rq = jp.render_params(W, Hh, 2, 4, 5, integrator=integ)
        assert same(_base(sp, rq)[0], _feat(sp, rq)[0])


def _one_lit(be, m):
    scenes.lamp_rect()(be, m)
    be.pointlight((278, 273, -200), (0.0, 0.0, 0.0))


def test_power_sampling_with_one_lit_light_is_all_sampling():
    """pmf (1, 0): the division by the pmf changes no bit, and under the debug sampler the two extra draws move nothing"""
    W = Hh = 32
    be = scenes.build_lamp_box(scenes.HostBackend("one_lit"), W, Hh, _one_lit, full_materials=True)
    sp = be.flatten()
    rp = jp.render_params(W, Hh, 2, DEPTH, 1, sampler_mode=jp.JP_SAMPLER_DEBUG)
    a, ca = _base(sp, rp)
    f = H.oracle_features(sp, "power")
    assert np.array_equal(f.table[3], np.array([1, 0], f32))
    b, cb, _ = H.oracle_render_features(sp, rp, f, 4)
    assert a.mean() > 0.02 and same(a, b) and _counts(ca) == _counts(cb)
    # MIS where every weight is 1: the counter sampler now, against power sampling with NEE (mirror and glass only around a delta light)
    be2 = scenes.HostBackend("delta_only")
    be2.camera((0, 1, 6), (0, 0, -1), (0, 1, 0), 50.0, W, Hh)
    be2.pointlight((0.5, 3.0, 1.0), (30.0, 28.0, 25.0)); be2.dirlight((0.2, -1.0, -0.3), (1.0, 0.9, 0.8))
    mm = be2.mat_matte((0.6, 0.5, 0.4)); mi = be2.mat_mirror((0.9, 0.9, 0.9)); gl = be2.mat_glass(1.5, (0.98,) * 3, (0.97,) * 3); me = be2.mat_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.15, 0.3, False)
    be2.rect(scenes.AXIS_XZ, -5, 5, -5, 5, 0.0, False, mm); be2.sphere((-1.2, 1.0, 0.0), 1.0, mi); be2.sphere((1.2, 0.8, 0.5), 0.8, gl); be2.disk((0.0, 0.6, -2.0), (0.0, 0.4, 1.0), 1.2, me)
    be2.preprocess()
    sp2 = be2.flatten()
    rq = jp.render_params(W, Hh, 8, DEPTH, 3)
    n, cn, _ = _feat(sp2, rq, light_mode="power")
    m, cm, _ = _feat(sp2, rq, light_mode="power", estimator="mis")
    assert n.mean() > 0.02 and same(n, m) and _counts(cn) == _counts(cm)


def test_constant_map_is_the_constant_environment_light_where_the_definitions_coincide():
    """a 1 x 1 map of (1, 1, 1) tinted by the light's radiance: a miss adds the same colour.  The two definitions sample the sky differently (uniform in
    (theta, phi) against uniform in solid angle), so they coincide exactly where the sky is only looked up: max_depth 0, and any depth in a scene of delta
    materials; the light table is the same either way (mean_sum of the constant map is the radiance sum)."""
    W, Hh = 32, 24
    be = scenes.HostBackend("const_map")
    be.camera((0, 1, 6), (0, 0, -1), (0, 1, 0), 50.0, W, Hh)
    be.envlight((0.3, 0.4, 0.6))
    mi = be.mat_mirror((0.9, 0.85, 0.8)); gl = be.mat_glass(1.5, (0.98,) * 3, (0.97,) * 3)
    be.sphere((-1.2, 1.0, 0.0), 1.0, mi); be.sphere((1.2, 0.8, 0.5), 0.8, gl); be.rect(scenes.AXIS_XZ, -5, 5, -5, 5, 0.0, False, mi)
    be.preprocess()
    sp = be.flatten()
    one = np.ones((1, 1, 3), f32)
    for depth in (0, DEPTH):
        rp = jp.render_params(W, Hh, 4, depth, 11)
        a, ca = _base(sp, rp)
        f = H.oracle_features(sp, "power", env_rgb=one, env_up="y")
        g = H.oracle_features(sp, "power")
        assert np.array_equal(f.table[1], g.table[1]) and np.array_equal(f.table[3], g.table[3]) and abs(f.table[0][0] / g.table[0][0] - 1) < 1e-12
        b, cb, und = H.oracle_render_features(sp, rp, f, 4)
        assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb) and not und.any()
        m, cm, _ = _feat(sp, rp, light_mode="power", env_rgb=one, env_up="y", estimator="mis")
        assert same(a, m)


def test_neutral_states_change_nothing_on_the_zoo():
    """on the matrix's own room: a constant texture equal to the constant colour, neutral normal maps and strength 0, identity sampling records, lens radius 0
    and the zero film state give the film without them, in JP_LIGHTS_ALL against jp_oracle_render and in the richest family against itself"""
    be = build_zoo("zoo")
    sp = be.flatten(); s = sp.contents
    rp = jp.render_params(32, 24, 8, DEPTH, 5)
    a, ca = _base(sp, rp)
    mt = np.ctypeslib.as_array(s.mat_type, (s.n_materials,)); mp = np.ctypeslib.as_array(s.mat_params, (16 * s.n_materials,)).reshape(-1, 16)
    ok = np.isin(mt, (0, 1, 3))                                    # matte, mirror, plastic may carry a texture
    flat_map = np.full((4, 4, 3), 128, np.uint8); flat_map[..., 2] = 255
    bumpy = _nmap_image()
    ident = jp.texture_sampling(tex=[jp.tex_sampler()] * int(ok.sum()), maps=[jp.tex_sampler(), jp.tex_sampler()])
    neutral = dict(normal_maps=jp.normal_maps([flat_map, bumpy], np.where(np.arange(s.n_materials) % 2 == 0, 0, 1), np.where(np.arange(s.n_materials) % 2 == 0, 1.0, 0.0).astype(f32)),
                   sampling=ident, lens=jp.lens(0.0), film=jp.film(0, 0.0))
    # (a textured plastic recomputes Qd from the sampled Kd in fp32: the constructor's value only up to its own rounding, so plastic keeps its own colour here)
    solid2 = jp.textures([jp.JP_TEXTURE_SOLID] * int(ok.sum()), [tuple(mp[i, :3]) + (0, 0, 0) for i in np.flatnonzero(ok)],
                         np.where(ok & (mt != 3), np.cumsum(ok) - 1, -1), s.n_triangles)
    b, cb, und = _feat(sp, rp, **dict(neutral, textures=solid2))
    assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb) and not und.any()
    rich = dict(light_mode="power", env_rgb=env_map_rgb(), env_up="y", estimator="mis", normals=jp.vertex_normals(zoo_vertex_normals(s)))
    c, cc, _ = _feat(sp, rp, **rich)
    d, cd, _ = _feat(sp, rp, **dict(rich, **dict(neutral, textures=solid2)))
    assert c.mean() > 0.05 and same(c, d) and _counts(cc) == _counts(cd) and not same(a, c)


def test_film_does_not_depend_on_the_thread_count():
    st, film, cnt, und = oracle_of("zoo", "smooth_mis_env_tex_extras")
    for nt in (0, 1, 3):
        f2, c2, u2 = H.oracle_render_features(st["sp"], st["params"], st["features"], nt)
        assert same(film, f2) and _counts(cnt) == _counts(c2) and cnt.samples == c2.samples and np.array_equal(und, u2)


# ---- 2. the undecided share of every cell of the GPU matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,family", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_undecided_share_is_at_most_one_percent(variant, family):
    st, film, cnt, und = oracle_of(variant, family)
    W, Hh = SIZES[variant]
    print("%s / %s: %d of %d pixels undecided, film mean %.4f, %d closest rays, %d shadow rays" % (variant, family, und.sum(), und.size, film.mean(), cnt.closest_rays, cnt.shadow_rays))
    assert np.isfinite(film).all() and film.mean() > 0.05 and cnt.samples == W * Hh * SPP
    assert und.mean() <= 0.01
    fam = FAMILIES[family]
    if not fam["env"] and not fam["tex"] and not fam["nmap"]:
        assert not und.any()                                       # no lookup through acosf / atan2f / asinf: nothing can be undecided


@pytest.mark.parametrize("variant", sorted(ROWS))
def test_variants_reach_their_rows(variant):
    """jp_describe_upload (pure host code): what the upload plans for each variant, in both light sampling modes"""
    be = scene_of(variant, FAMILIES["all"])
    s = be.flatten().contents
    for k, mode in enumerate(("all", "power")):
        i = jp.describe_upload(be.flatten(), None, mode)
        print("%s, %s: %d primitives, %d lights, %d shadow planes; tables in LDS %d, records in LDS %d, staged %d; sort %d, null material %d, masks %x %x %x %x" % (
            variant, mode, s.n_primitives, s.n_lights, i.n_planes, i.tables_in_lds, i.shade_prims_in_lds, i.stage_nee, i.shade_sort, i.has_null_material, i.class_mask, i.shape_mask, i.light_mask, i.light_shape_mask))
        assert (i.tables_in_lds, i.shade_prims_in_lds, i.stage_nee) == ROWS[variant][k] and i.trav_mode == 5
    lean = variant.startswith("cornell")                            # jp_render.h lean_shading: flat shapes, area lights on them, matte / metal only, records in LDS, staged
    i = jp.describe_upload(be.flatten(), None, "all")
    flat = (i.shape_mask & ~((1 << 0) | (1 << 1))) == 0 and (i.light_shape_mask & ~((1 << 0) | (1 << 1))) == 0
    assert (flat and (i.light_mask & ~(1 << 1)) == 0 and (i.class_mask & ((2 << 1) | (2 << 2) | (2 << 3))) == 0) == lean
    assert i.has_null_material == (0 if variant in ("zoo_few", "zoo_bulk_few", "cornell") else 1)


def test_feature_sets_differ():
    """the families of one room are different films (a feature that silently did nothing would make two of them equal), with the same ray counts for NEE and MIS"""
    films = {f: oracle_of("zoo", f)[1] for v, f in GROUPS if v == "zoo"}
    names = sorted(films)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not same(films[a], films[b]), (a, b)
    for f in names:
        if FAMILIES[f]["est"] == "mis" and not f.endswith("_extras") and not (FAMILIES[f]["mip"] or FAMILIES[f]["proc"]):   # (the cone families have no NEE twin in the matrix)
            nee = f.replace("mis_env", "env").replace("mis", "pick")
            assert _counts(oracle_of("zoo", f)[2]) == _counts(oracle_of("zoo", nee)[2]), f


def test_refused_combinations_are_refused():
    st = state_of("zoo", FAMILIES["all"])
    for kw in (dict(light_mode="all", estimator="mis"), dict(light_mode="all", env_rgb=env_map_rgb(), env_up="y")):
        with pytest.raises(jp.JetPbrtError) as e:
            H.oracle_render_features(st["sp"], st["params"], H.oracle_features(st["sp"], **kw), 2)
        assert "status -5" in str(e.value)                         # JP_ERR_UNSUPPORTED: both need the light table
    rw = jp.render_params(32, 24, 1, 3, 1, integrator=jp.JP_INTEGRATOR_WHITTED)
    for kw in (dict(light_mode="power"), dict(normals=jp.vertex_normals(zoo_vertex_normals(st["sp"].contents)))):
        with pytest.raises(jp.JetPbrtError):
            H.oracle_render_features(st["sp"], rw, H.oracle_features(st["sp"], **kw), 2)


# ---- 3. NEE against MIS ---------------------------------------------------------------------------------------------------------------------------------------
def test_nee_and_mis_agree_in_the_mean():
    """one scene where neither strategy is degenerate (the room with every light one-sided: large and small emitters, glossy and matte surfaces, the map), on the
    unclamped film (Clamp01 biases a mean, and leaving clamped pixels out selects against the noisier estimator).  Per seed the difference of the two films' image
    means; its mean over the seeds against its standard error, from the sample variance of the oracle films themselves."""
    fam_n = dict(FAMILIES["env_tex"], film=True); fam_m = dict(FAMILIES["mis_env_tex"], film=True)
    st_n = state_of("zoo_one_sided", fam_n); st_m = state_of("zoo_one_sided", fam_m)
    hdr = jp.film(1, 0.0)
    fn = H.oracle_features(st_n["sp"], "power", st_n["rgb"], "y", 0, "nee", textures=st_n["textures"], film=hdr)
    fm = H.oracle_features(st_m["sp"], "power", st_m["rgb"], "y", 0, "mis", textures=st_m["textures"], film=hdr)
    n_seeds, spp = 12, 64
    dn, mn = [], []
    for k in range(n_seeds):
        rp = jp.render_params(32, 24, spp, DEPTH, 7000 + 13 * k)
        a = H.oracle_render_features(st_n["sp"], rp, fn, 8)[0].astype(np.float64); b = H.oracle_render_features(st_m["sp"], rp, fm, 8)[0].astype(np.float64)
        dn.append(a.mean() - b.mean()); mn.append(a.mean())
    dn = np.array(dn)
    se = dn.std(ddof=1) / np.sqrt(n_seeds)
    z = dn.mean() / se
    print("NEE - MIS: mean difference %.3e (image mean %.4f), standard error %.3e, z = %+.2f" % (dn.mean(), np.mean(mn), se, z))
    assert abs(z) <= 4.0                                             # 6e-5 two-sided for unbiased estimators
    assert se < 0.01 * np.mean(mn)                                   # ... and sharp enough to see a missing pmf or a swapped weight: those move the mean by several per cent


# ---- 4. closed forms: the scenes, sample counts and bounds of the GPU tests of the features, met by the oracle --------------------------------------------------
def test_delta_light_predictor_on_the_smooth_icosphere():
    """tests/test_gpu_normals.py test_direct_light_of_a_delta_light_equals_the_predictor, its scene and bounds: within 1e-5 of normals_ref.direct_delta on every
    hit pixel the predictor does not mark fragile, for the families all / power / mis / textured"""
    import test_gpu_normals as G
    for family, fam in sorted(G.FAMILIES.items()):
        be = G._ico_scene(1, 48, tex=fam["tex"])
        sp = be.flatten(); s = sp.contents
        vn = R.radial_normals(s)
        f = H.oracle_features(sp, fam["mode"], estimator=fam["est"], normals=jp.vertex_normals(vn), textures=be.flatten_textures() if fam["tex"] else None)
        rp = jp.render_params(48, 48, 1, 1, 7, sampler_mode=jp.JP_SAMPLER_DEBUG)
        film, _, _ = H.oracle_render_features(sp, rp, f, 4)
        o, d = R.camera_rays(s)
        if fam["tex"]:
            p = o + _first_hit_t(sp, o, d)[:, None] * d
            sgn = np.sin(10 * p[:, 0].astype(f32)) * np.sin(10 * p[:, 1].astype(f32)) * np.sin(10 * p[:, 2].astype(f32))
            alb = np.where((sgn < 0)[:, None], 0.6, 0.3) * np.ones(3)
        else:
            alb = np.full((len(d), 3), 0.6)
        pred, hit, fragile, n_only, g_only = R.direct_delta(s, vn, alb)
        flat = R.direct_delta(s, vn, alb, use_ng=True)[0]
        keep = hit & ~fragile
        err = np.abs(film.astype(np.float64) - pred).max(-1)
        print("%s: %d hit pixels, %d fragile, largest error %.3e" % (family, hit.sum(), fragile.sum(), err[keep].max()))
        assert hit.sum() > 700 and fragile.sum() <= 0.02 * hit.sum()
        assert (film[~hit] == 0).all()
        assert err[keep].max() <= 1e-5
        assert np.abs(film.astype(np.float64) - flat).max(-1)[hit].mean() > 0.01


def _first_hit_t(sp, o, d):
    L = H.oracle_lib()
    h = H.oracle_scene(L, sp)
    n = len(d)
    o32 = np.ascontiguousarray(o, f32); d32 = np.ascontiguousarray(d, f32)
    hit = np.zeros(n, np.int32); t = np.zeros(n, f32); prim = np.zeros(n, np.int32); nrm = np.zeros((n, 3), f32); pos = np.zeros((n, 3), f32)
    L.jp_oracle_trace(h, n, H.ptr(o32), H.ptr(d32), H.ptr(np.full(n, 1e-3, f32)), H.ptr(np.full(n, np.inf, f32)), H.ptr(hit), H.ptr(t), H.ptr(prim), H.ptr(nrm), H.ptr(pos))
    L.jp_oracle_scene_free(h)
    return np.where(hit != 0, t, 0.0).astype(np.float64)


def _z_of(films, expected):
    """tests/test_gpu_mis.py _z_scores: no pixel clamped, the image mean of eight films against the closed form in units of its standard error"""
    assert max(float(f.max()) for f in films) < 0.99
    means = np.array([f.astype(np.float64).mean((0, 1)) for f in films])
    se = means.std(0, ddof=1) / np.sqrt(len(films))
    z = (means.mean(0) - expected) / se
    print("image mean %s vs closed form %s: z = %s" % (np.array2string(means.mean(0), precision=6), np.array2string(np.asarray(expected), precision=6), np.array2string(z, precision=2)))
    return z


@pytest.mark.parametrize("est", ["nee", "mis"])
def test_polygon_formula_under_a_rectangle_light(est):
    """tests/test_gpu_mis.py test_unbiased_against_the_polygon_formula: its scene, 8 films of 32 x 32 at 128 spp and depth 1, seeds 1000 + 17 k, |z| <= 5"""
    import test_gpu_mis as G
    Le = np.array([6.0, 5.0, 4.0])
    be = G._floor_under_rect(Le)
    sp = be.flatten(); s = sp.contents
    lamp = [sh for sh in M.shapes_of(s) if sh["light"] >= 0][0]
    assert lamp["n"][1] < 0
    pts = G._floor_points(s.camera)
    irr = M.polygon_irradiance(M.rect_corners(lamp), pts.reshape(-1, 3), np.array([0.0, 1.0, 0.0])).reshape(G.Hh, G.W, -1).mean(-1)
    expected = (np.asarray(G.KD)[None, None] / np.pi * Le[None, None] * irr[..., None]).mean((0, 1))
    f = H.oracle_features(sp, "power", estimator=est)
    films = [H.oracle_render_features(sp, jp.render_params(G.W, G.Hh, 128, 1, 1000 + 17 * k), f, 8)[0] for k in range(8)]
    assert (np.abs(_z_of(films, expected)) <= 5.0).all()


@pytest.mark.parametrize("est", ["nee", "mis"])
def test_closed_form_under_the_map(est):
    """tests/test_gpu_envmap.py test_unbiased_against_closed_form (nee) and tests/test_gpu_mis.py test_unbiased_under_the_map (mis): a matte floor under
    envmap_ref.bright_map() against envmap_ref.floor_closed_form, 8 films of 32 x 32 at 128 spp and depth 1, seeds 1000 + 17 k, |z| <= 5"""
    import envmap_ref as E
    import test_gpu_mis as G
    be = scenes.HostBackend("oracle_floor_map")
    be.camera((0, 5, 0), (0, -1, 0), (0, 0, -1), 40.0, G.W, G.Hh)
    be.envlight((1.0, 1.0, 1.0))
    be.rect(scenes.AXIS_XZ, -50, 50, -50, 50, 0.0, False, be.mat_matte(G.KD))
    be.preprocess()
    sp = be.flatten()
    rgb = E.bright_map()
    rgb = (rgb * f32(0.559 / E.floor_closed_form(rgb, (1, 1, 1), G.KD).max())).astype(f32)
    expected = E.floor_closed_form(rgb, (1, 1, 1), G.KD)
    f = H.oracle_features(sp, "power", env_rgb=rgb, env_up="y", estimator=est)
    films = [H.oracle_render_features(sp, jp.render_params(G.W, G.Hh, 128, 1, 1000 + 17 * k), f, 8)[0] for k in range(8)]
    assert (np.abs(_z_of(films, expected)) <= 5.0).all()


GOLDEN_66 = os.path.join(H.GOLDEN, "oracle_66_lights_all_4096spp.npy")


def make_golden_66():
    """python -c "import sys; sys.path.insert(0, 'tests'); import test_oracle_features_host as T; T.make_golden_66()": the reference film R of the 66-light test,
    jp_oracle_render in JP_LIGHTS_ALL at 4096 spp (66 shadow rays a bounce: five minutes of CPU, which is why it is a fixture)"""
    import test_gpu_light_pick as G
    be = G._box(scenes.lamp_66)
    np.save(GOLDEN_66, H.oracle_render(be.flatten(), jp.render_params(G.W, G.Hh, G.R_SPP, 5, 7), len(os.sched_getaffinity(0)))[0])


def test_66_lights_against_all_sampling():
    """tests/test_gpu_light_pick.py test_66_lights_unbiased, its scene, sample counts and bounds: the reference R is JP_LIGHTS_ALL at 4096 spp (seed 7:
    jp_oracle_render's film, committed as a fixture by make_golden_66 and re-rendered here on one band of four rows, bit for bit); power sampling's mean per-pixel L2
    to it falls as an unbiased estimator's does (e(1024) <= 0.35 e(64), seed 99) and the image mean of eight films at 128 spp (seeds 1000 + 17 k) is within 5
    standard errors of R's, over the pixels nothing clamps (at most 15 % left out)"""
    import test_gpu_light_pick as G
    be = G._box(scenes.lamp_66)
    sp = be.flatten()
    assert sp.contents.n_lights == 66
    nt = len(os.sched_getaffinity(0))
    Rf = np.load(GOLDEN_66)
    band = H.oracle_render(sp, jp.render_params(G.W, G.Hh, G.R_SPP, 5, 7, band_rows=4, shard_index=5, shard_count=12), nt)[0]
    assert band[20:24].mean() > 0.02 and same(band[20:24], Rf[20:24]) and (band[:20] == 0).all() and (band[24:] == 0).all()
    f = H.oracle_features(sp, "power")
    G.check_table(*f.table)
    film = lambda spp, seed: H.oracle_render_features(sp, jp.render_params(G.W, G.Hh, spp, 5, seed), f, nt)[0]
    assert 1.0 - (Rf < 0.99).all(-1).mean() <= 0.15
    e = {}
    for spp in (64, 1024):
        e[spp], out = G._l2(film(spp, 99), Rf)
        assert out <= 0.15
    films = [film(128, 1000 + 17 * k) for k in range(8)]
    keep = (Rf < 0.99).all(-1)
    for g in films:
        keep &= (g < 0.99).all(-1)
    assert 1.0 - keep.mean() <= 0.15
    means = np.array([g[keep].astype(np.float64).mean() for g in films]); rmean = Rf[keep].astype(np.float64).mean()
    z = (means.mean() - rmean) / (means.std(ddof=1) / np.sqrt(8.0))
    print("66 lights: e(64) = %.5f, e(1024) = %.5f, ratio %.3f; image mean %.6f vs R %.6f, z = %+.2f (left out %.3f)" % (e[64], e[1024], e[1024] / e[64], means.mean(), rmean, z, 1.0 - keep.mean()))
    assert e[1024] <= 0.35 * e[64] and abs(z) <= 5.0


# ---- 5. the ray cone: mip maps and procedural textures (INTEGRATION.md sections 18, 19) ----------------------------------------------------------------------
def _cone_render(st, **over):
    """the oracle on a state of the matrix with its textures / mipmaps / procedurals replaced -> (film, counters, undecided, branch statistics)"""
    kw = dict(textures=st["textures"], mipmaps=st["mipmaps"], procedurals=st["procedurals"])
    kw.update(over)
    f = H.oracle_features(st["sp"], st["mode"], st["rgb"], "y", 0, st["est"], None if st["vn"] is None else jp.vertex_normals(st["vn"]), kw["textures"], st["sampling"],
                          st["nmaps"], st["lens"], st["film"], mipmaps=kw["mipmaps"], procedurals=kw["procedurals"])
    stats = H.JpOracleBranchStats()
    film, cnt, und = H.oracle_render_features(st["sp"], st["params"], f, 8, stats=stats)
    return film, cnt, und, stats.arrays(), f


def _mip_lookups(a):
    return a["mip_rho_zero"] + a["mip_rho_le1"] + a["mip_two_level"].sum(1) + a["mip_last_level"]


def test_cone_state_that_is_off_is_the_film_without_it():
    """all modes OFF and all kinds NONE -- whatever footprint_scale and bounce_spread say -- and the struct of before this state (a shorter struct_bytes: absent)"""
    st = state_of("zoo", FAMILIES["mis_env_tex_mip_proc"])
    n = st["textures"].contents.n_textures
    a, ca, ua, sa, _ = _cone_render(st, mipmaps=None, procedurals=None)
    b, cb, ub, sb, _ = _cone_render(st, mipmaps=jp.texture_mipmaps([jp.JP_MIP_OFF] * n, 3.0, 0.3), procedurals=jp.texture_procedurals([None] * n))
    assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb) and np.array_equal(ua, ub)
    assert all(int(v.sum()) == 0 for v in sb.values())
    f = _cone_render(st)[4]
    f.struct_bytes = H.JpOracleFeatures.mipmaps.offset
    c, cc, uc = H.oracle_render_features(st["sp"], st["params"], f, 8)
    assert same(a, c) and _counts(ca) == _counts(cc) and np.array_equal(ua, uc)
    d = oracle_of("zoo", "mis_env_tex_mip_proc")[1]
    assert not same(a, d)


def test_mipmaps_on_a_1x1_image_change_nothing():
    """every level of a 1 x 1 image is its texel: level L - 1 = 0 alone, whatever the footprint"""
    be = build_zoo("zoo")
    sp = be.flatten(); s = sp.contents
    mt = np.ctypeslib.as_array(s.mat_type, (s.n_materials,))
    tex = jp.textures([jp.JP_TEXTURE_IMAGE], [(0,) * 6], np.where(np.isin(mt, (0, 1)), 0, -1), s.n_triangles, images={0: np.array([[[200, 90, 40]]], np.uint8)})
    rp = jp.render_params(32, 24, 8, DEPTH, 5)
    a, ca, _ = H.oracle_render_features(sp, rp, H.oracle_features(sp, "all", textures=tex), 4)
    stats = H.JpOracleBranchStats()
    b, cb, _ = H.oracle_render_features(sp, rp, H.oracle_features(sp, "all", textures=tex, mipmaps=jp.texture_mipmaps([jp.JP_MIP_TRILINEAR], 50.0)), 4, stats=stats)
    k = stats.arrays()
    assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb)
    assert k["mip_last_level"].sum() > 1000 and k["mip_two_level"].sum() == 0


def test_a_footprint_below_one_texel_is_the_film_without_mipmaps():
    """footprint_scale so small that every rho <= 1: the lookup the texture has without mipmaps, under a sampling record (the floor) and without one (the back wall)"""
    st = state_of("zoo", FAMILIES["mis_env_tex_mip"])
    a, ca, ua, _, _ = _cone_render(st, mipmaps=None)
    b, cb, ub, k, _ = _cone_render(st, mipmaps=zoo_mipmaps(st["be"], footprint_scale=1e-6))
    assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb) and np.array_equal(ua, ub)
    assert k["mip_rho_le1"].sum() > 1000 and k["mip_two_level"].sum() == 0 and k["mip_last_level"].sum() == 0
    assert not same(a, oracle_of("zoo", "mis_env_tex_mip")[1])


def test_equal_colours_under_any_record_give_the_solid_colours_film():
    """tests/test_gpu_procedural.py test_equal_colours_give_the_film_of_the_solid_texture, on the oracle: both colours (1 / 255) b, so r = c whatever t is and
    (1 / 255) b is the colour the byte b stands for; the plain-checker word of CHECKER_AA names an entry of the colour table, the same colour"""
    import test_gpu_procedural as G
    st = state_of("zoo", FAMILIES["pick_tex_proc"])
    src = st["textures"].contents
    types = np.array([src.tex_type[k] for k in range(src.n_textures)], np.int32)
    colors = np.array([src.tex_color[k] for k in range(6 * src.n_textures)], f32).reshape(-1, 6)
    checkers = np.flatnonzero(types == jp.JP_TEXTURE_CHECKER)
    assert len(checkers) == len(proc_records())
    rng = np.random.default_rng(5)
    for k in checkers:
        c = (f32(1.0) / f32(255.0)) * rng.integers(40, 230, 3).astype(f32)
        colors[k, :3] = c; colors[k, 3:] = c
    solid = types.copy(); solid[checkers] = jp.JP_TEXTURE_SOLID
    a, ca, _, k, _ = _cone_render(st, textures=G._copy_textures(st["textures"], types, colors))
    b, cb, _, _, _ = _cone_render(st, textures=G._copy_textures(st["textures"], solid, colors), procedurals=None)
    assert a.mean() > 0.05 and same(a, b) and _counts(ca) == _counts(cb)
    assert k["checker_plain"].sum() > 0 and k["checker_filtered"].sum() > 0 and k["proc_partial"].sum() > 0
    assert not same(a, oracle_of("zoo", "pick_tex_proc")[1])


@pytest.mark.parametrize("which", ["direct", "mirror", "matte"])
def test_saturating_constructions_of_the_mipmap_tests(which):
    """tests/test_gpu_mipmap.py's three exact films (direct view, a width carried across a mirror, a spread widened by a diffuse bounce), their scenes and
    parameters: the oracle's mip film equals the oracle's film of the constant grey image, and the image without mipmaps does not"""
    import test_gpu_mipmap as G
    build, img, scale, spread = {"direct": (G._scene_direct, G._checker(64, 1), 4.0, 0.125), "mirror": (G._scene_mirror, G._checker(64, 2), 8.0, 1.0),
                                 "matte": (G._scene_matte, G._checker(64, 2), 4.0, 0.5)}[which]
    rp = jp.render_params(G.W, G.H, 4, 4, 1234)
    films = []
    for im, mip in ((img, [1]), (img, None), (G.GREY, None)):
        be = build(im, scale)
        sp = be.flatten()
        f = H.oracle_features(sp, textures=be.flatten_textures(), sampling=be.flatten_texture_sampling(), mipmaps=None if mip is None else jp.texture_mipmaps(mip, bounce_spread=spread))
        films.append(H.oracle_render_features(sp, rp, f, 4)[0])
    a, b, c = films
    assert a.mean() > 0.01 and same(a, c) and not same(b, c) and np.abs(b - c).max() > 0.02


@pytest.mark.parametrize("variant,family", CONE_GROUPS, ids=["%s-%s" % g for g in CONE_GROUPS])
def test_new_groups_reach_every_branch(variant, family):
    """conditions on the inputs (MIP_SIZES, MIP_FOOTPRINT, MIP_SPREAD, proc_records were chosen until they held), from the oracle's branch statistics: a cell whose
    lookups all took one branch would pin nothing of the others"""
    fam = FAMILIES[family]
    a = oracle_of(variant, family)[0]["stats"].arrays()
    print("%s / %s: %s" % (variant, family, {k: v.tolist() for k, v in a.items() if k != "mip_two_level"}), a["mip_two_level"].sum(0).tolist())
    mip = _mip_lookups(a)
    if fam["mip"]:
        n = int(mip.sum())
        assert n > 5000
        for k in ("mip_rho_le1", "mip_two_level", "mip_last_level"):
            assert a[k].sum() >= 0.02 * n, k
        assert (a["mip_two_level"].sum(0) > 0).sum() >= 3
        assert mip[1] >= 0.25 * n
    else:
        assert mip.sum() == 0
    for k in ("proc_all_one", "proc_partial", "proc_early"):
        assert a[k][0].sum() == 0 and a[k][jp.JP_PROC_CHECKER_AA].sum() == 0
    by_kind = a["proc_all_one"] + a["proc_partial"] + a["proc_early"]
    checker = a["checker_plain"] + a["checker_filtered"] + a["checker_half"]
    if not fam["proc"]:
        assert by_kind.sum() == 0 and checker.sum() == 0
    else:
        for kind in (jp.JP_PROC_NOISE, jp.JP_PROC_FBM, jp.JP_PROC_TURBULENCE, jp.JP_PROC_MARBLE):
            assert by_kind[kind].sum() > 0, kind
        assert checker.sum() > 0
        if fam["proc"] == "off":                                   # no footprint: every octave at weight 1, the plain checker's word everywhere
            assert a["proc_partial"].sum() == 0 and a["proc_early"].sum() == 0 and a["checker_filtered"].sum() == 0 and a["checker_half"].sum() == 0
        else:
            for kind in (jp.JP_PROC_FBM, jp.JP_PROC_TURBULENCE):
                for k in ("proc_all_one", "proc_partial", "proc_early"):
                    assert a[k][kind].sum() >= 50, (kind, k)
            for k in ("checker_plain", "checker_filtered", "checker_half"):
                assert a[k].sum() >= 50, k
            assert by_kind[:, 1].sum() + checker[1] >= 0.25 * (by_kind.sum() + checker.sum())


@pytest.mark.parametrize("family", ["mis_env_tex_mip", "pick_tex_proc", "mis_env_tex_mip_proc"])
def test_the_film_sees_the_cone_beyond_the_first_hit(family):
    """only bounce_spread changes (0.125 -> 0.25; the procedural family carries it in a mipmap state whose modes are all OFF): the first segment's cone is
    gamma0 t whatever the spread, so every first-hit lookup keeps its branch and its word; the film changes, so the matrix sees the state the paths carry"""
    st = state_of("zoo", FAMILIES[family])
    mk = (lambda s: zoo_mipmaps(st["be"], bounce_spread=s)) if FAMILIES[family]["mip"] else (lambda s: zoo_mipmaps(st["be"], 0.0, s, on=()))
    a, ca, _, ka, _ = _cone_render(st, mipmaps=mk(0.125))
    b, cb, _, kb, _ = _cone_render(st, mipmaps=mk(0.25))
    assert not same(a, b)
    for k in ka:
        first_a, first_b = ka[k][..., 0] if k != "mip_two_level" else ka[k][0], kb[k][..., 0] if k != "mip_two_level" else kb[k][0]
        assert np.array_equal(first_a, first_b), k
    assert ka["word_sum"][0] > 0 and ka["word_sum"][1] != kb["word_sum"][1]
    # 0 means the default, 0.125
    c = _cone_render(st, mipmaps=mk(0.0))[0]
    assert same(a, c)


def test_cone_film_does_not_depend_on_the_thread_count():
    st, film, cnt, und = oracle_of("zoo", "smooth_mis_env_tex_mip_proc_extras")
    ref = st["stats"].arrays()
    for nt in (0, 1, 3):
        k = H.JpOracleBranchStats()
        f2, c2, u2 = H.oracle_render_features(st["sp"], st["params"], st["features"], nt, stats=k)
        assert same(film, f2) and _counts(cnt) == _counts(c2) and cnt.samples == c2.samples and np.array_equal(und, u2)
        assert all(np.array_equal(v, ref[n]) for n, v in k.arrays().items())
