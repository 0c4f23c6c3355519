"""The host half of jp_upload_scene (csrc/jp_scene_host.h: check_scene, the table builders, plan_scene) through jp_describe_upload: no GPU needed.

tests/golden/upload_describe.json holds, per case, every field of JpUploadInfo: the plan the upload decides on, and byte count and FNV-1a of every table it
hands to the device.  It was recorded from the commit BEFORE the upload was split into builders (that commit's jp_upload_scene, instrumented to hash inside
upload() and to skip its device calls), so equality here means: same plan, same bytes as the one-function upload produced.  The refusals are matched against
the messages of that commit's source as well.  tests/test_gpu_upload_describe.py ties the description to what a real upload reports."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import harness as H

W, HH = 32, 24
GOLDEN = os.path.join(H.GOLDEN, "upload_describe.json")
RANDOM = dict(seed=7, n_tris=1600)

# name -> (scene, reference tree: None / "verbatim" / "certified", JpOptions fields, light mode)
CASES = {
    "cornell": ("cornell", None, {}, "all"),
    "cornell_lambert": ("cornell_lambert", None, {}, "all"),
    "misc": ("misc", None, {}, "all"),
    "lights": ("lights", None, {}, "all"),
    "disks": ("disks", None, {}, "all"),
    "bunny_small": ("bunny_small", None, {}, "all"),
    "bunny_small_reference": ("bunny_small", "verbatim", {}, "all"),
    "bunny_small_certified": ("bunny_small", "certified", {}, "all"),
    "random_1600": ("random", None, {}, "all"),
    "random_1600_certified": ("random", "certified", {}, "all"),
    "cornell_power_one": ("cornell", None, {}, "power"),
    "random_1600_traversal_0": ("random", None, dict(traversal=1), "all"),
    "random_1600_traversal_1": ("random", None, dict(traversal=2), "all"),
    "random_1600_traversal_3": ("random", None, dict(traversal=4), "all"),
    "random_1600_no_q4": ("random", None, dict(q4=-1), "all"),
    # forty emitting triangles, 70 primitives: the one scene here that is walked as a binary tree in LDS (mode 1), and more shadow planes than k_shade stages
    "lamp_grid_40": ("lamp_grid", None, {}, "all"),
}
INT_FIELDS = [n for n, t in jp.JpUploadInfo._fields_ if t in (C.c_int32, C.c_int64) and n != "struct_bytes"]
FLOAT_FIELDS = ["cert_pad", "cert_pad_eye"]


def build_case(name, tmpdir):
    """-> (backend, keeping the arrays alive; pointer to its JpScene; JpOptions or None; light mode)"""
    scene, tree, opts, mode = CASES[name]
    be = scenes.HostBackend(name)
    if tree:
        be.set_reference_tree(True, certified=(tree == "certified"))
    if scene == "random":
        H.build_random_scene(be, W, HH, tmpdir=str(tmpdir), **RANDOM)
    elif scene == "lamp_grid":
        scenes.build_lamp_box(be, W, HH, scenes.lamp_mesh(5, 4))
    else:
        H.SCENES[scene](be, W, HH)
    o = None
    if opts:
        o = jp.JpOptions(); o.struct_bytes = C.sizeof(jp.JpOptions)
        for k, v in opts.items():
            setattr(o, k, v)
    return be, be.flatten(), o, mode


def info_dict(i):
    """a JpUploadInfo in the golden file's form"""
    d = {n: int(getattr(i, n)) for n in INT_FIELDS}
    d.update({n: float(getattr(i, n)) for n in FLOAT_FIELDS})
    d.update({"env_sum_" + c: float(i.env_sum[k]) for k, c in enumerate("rgb")})
    d["tables"] = {n: [int(i.table[k].bytes), "%016x" % i.table[k].fnv1a] for k, n in enumerate(jp.UPLOAD_TABLES)}
    return d


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def described(tmp_path_factory):
    d = tmp_path_factory.mktemp("upload_host")
    out = {}
    for name in CASES:
        be, sp, o, mode = build_case(name, d)
        out[name] = info_dict(jp.describe_upload(sp, o, mode))
        be.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_and_tables_are_the_one_function_uploads(name, described, golden):
    got, want = described[name], golden[name]
    assert set(got) == set(want)
    for k in sorted(got):
        if k == "tables":
            continue
        if k in INT_FIELDS:
            assert got[k] == want[k], k
        else:                                                           # floats: the golden holds %.9g, which names an fp32 value uniquely
            assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), k
    assert got["tables"] == want["tables"]


def test_the_cases_reach_every_path(golden):
    """from the recording, not from this tree: a golden full of flat-list scenes would prove nothing"""
    modes = {n: g["trav_mode"] for n, g in golden.items()}
    assert {0, 1} & set(modes.values()) and {2, 3, 5} <= set(modes.values())
    assert modes["random_1600_traversal_0"] == 0 and modes["random_1600"] == 3 and modes["bunny_small_reference"] == 5
    big = golden["random_1600"]
    assert big["n_prims"] > 1024 and big["use_q4"] == 1 and big["tables"]["wide"][0] > 0 and big["tables"]["q4"][0] > 0 and big["n_prims"] * 80 > 40 * 1024
    assert golden["random_1600_no_q4"]["use_q4"] == 0 and golden["random_1600_no_q4"]["tables"]["q4"] == [0, "0" * 16]
    cert = golden["random_1600_certified"]
    assert cert["cert"] == 1 and cert["trav_mode"] == 5 and cert["tables"]["refbox"][0] == 32 * cert["n_prims"] and cert["cert_pad"] > 0
    # the random scene's camera at (0, 0, 9) looks down -z at a floor, a back wall and soups of random triangles: some planes pass the eye
    assert cert["cert_eye_leaves"] > 0
    assert golden["bunny_small_certified"]["cert"] == 1 and golden["bunny_small_reference"]["cert"] == 0 and golden["bunny_small"]["n_prims"] > 1024
    assert golden["cornell"]["tables"]["flat"][0] > 0 and golden["random_1600"]["tables"]["flat"][0] == 0
    assert any(g["stage_nee"] == 0 or g["tables_in_lds"] == 0 for g in golden.values())
    assert modes["lamp_grid_40"] == 1 and golden["lamp_grid_40"]["n_planes"] == 40 and golden["cornell_power_one"]["n_planes"] == 1


# ---- the refusals of check_scene: same status, same jp_last_error text as the one-function upload ------------------------------------
def _cornell():
    be = scenes.build_cornell(scenes.HostBackend("refuse"), W, HH, lambert_only=False)
    return be, jp.JpScene.from_buffer_copy(be.flatten().contents)


def _own(s, keep, field, n, dtype, extra=0):
    """point s.<field> at a private copy of its first n elements (+ `extra` zeros) and return the copy"""
    ptr = getattr(s, field)
    a = np.concatenate([np.ctypeslib.as_array(ptr, (n,)).astype(dtype), np.zeros(extra, dtype)]) if n else np.zeros(extra, dtype)
    keep.append(a)
    setattr(s, field, a.ctypes.data_as(type(ptr)))
    return a


def _add_light(s, keep, kind):
    n = s.n_lights
    _own(s, keep, "light_type", n, np.int32, 1)[n] = kind
    _own(s, keep, "light_radiance", 3 * n, np.float32, 3)[3 * n:] = 1.0
    _own(s, keep, "light_prim", n, np.int32, 1)[n] = -1
    s.light_vec = None
    s.n_lights = n + 1


def _deep_tree(s, keep):
    """a chain of 40 interior nodes, each with a leaf to the left: height 40 (the leaves' contents are checked later)"""
    left = np.full(81, -1, np.int32); right = np.ones(81, np.int32)
    for i in range(40):
        left[i] = 40 + i; right[i] = i + 1 if i < 39 else 80
    b = np.zeros(6 * 81, np.float32)
    keep.extend([left, right, b])
    s.n_bvh_nodes = 81
    s.bvh_left = left.ctypes.data_as(type(s.bvh_left)); s.bvh_right = right.ctypes.data_as(type(s.bvh_right)); s.bvh_bounds = b.ctypes.data_as(type(s.bvh_bounds))


def _first_leaf(s):
    return next(n for n in range(s.n_bvh_nodes) if s.bvh_left[n] < 0)


def _set(field, value):
    return lambda s, keep: setattr(s, field, value)


def _poke(field, count, index, value, dtype=np.int32):
    def f(s, keep):
        _own(s, keep, field, count(s), dtype)[index(s) if callable(index) else index] = value(s) if callable(value) else value
    return f


def _lit_prim(s):
    return next(i for i in range(s.n_primitives) if s.prim_light[i] >= 0)


INVALID, UNSUPPORTED = -1, -5
REFUSALS = {
    "no_primitives": (_set("n_primitives", 0), "all", INVALID, "jp_upload_scene: scene has no primitives"),
    "negative_count": (_set("n_triangles", -1), "all", INVALID, "jp_upload_scene: negative count"),
    "reference_semantics_range": (_set("bvh_reference_semantics", 3), "all", INVALID, "jp_upload_scene: bvh_reference_semantics must be 0, 1 or 2"),
    "reference_semantics_without_tree": (lambda s, keep: (setattr(s, "bvh_reference_semantics", 1), setattr(s, "n_bvh_nodes", 0)), "all", INVALID,
                                         "jp_upload_scene: reference semantics need the caller's tree (n_bvh_nodes == 0)"),
    "null_array": (_set("prim_material", None), "all", INVALID, "jp_upload_scene: null array"),
    "null_array_for_count": (_set("mat_params", None), "all", INVALID, "jp_upload_scene: null array for a non-zero count"),
    "too_many_lights": (_set("n_lights", 256), "all", UNSUPPORTED, "jp_upload_scene: more than 255 lights are not supported by the shadow-entry packing"),
    "too_many_lights_power_one": (_set("n_lights", (1 << 24) + 1), "power", UNSUPPORTED, "jp_upload_scene: more than 2^24 lights (JP_LIGHTS_POWER_ONE)"),
    "shape_type": (_poke("prim_shape_type", lambda s: s.n_primitives, 0, 7), "all", INVALID, "jp_upload_scene: primitive shape reference out of range"),
    "shape_index": (_poke("prim_shape_index", lambda s: s.n_primitives, 0, 1 << 20), "all", INVALID, "jp_upload_scene: primitive shape reference out of range"),
    "material_index": (_poke("prim_material", lambda s: s.n_primitives, 0, lambda s: s.n_materials), "all", INVALID, "jp_upload_scene: primitive material out of range"),
    "light_index": (_poke("prim_light", lambda s: s.n_primitives, 0, lambda s: s.n_lights), "all", INVALID, "jp_upload_scene: primitive light out of range"),
    "light_not_area": (_poke("light_type", lambda s: s.n_lights, lambda s: s.prim_light[_lit_prim(s)], 0), "all", INVALID, "jp_upload_scene: primitive light is not an area light"),
    "material_type": (_poke("mat_type", lambda s: s.n_materials, 0, 9), "all", INVALID, "jp_upload_scene: unknown material type"),
    "area_light_prim": (_poke("light_prim", lambda s: s.n_lights, lambda s: s.prim_light[_lit_prim(s)], -1), "all", INVALID, "jp_upload_scene: area light primitive out of range"),
    "point_light_without_vec": (lambda s, keep: _add_light(s, keep, 2), "all", INVALID, "jp_upload_scene: point / direction light without light_vec"),
    "light_type": (lambda s, keep: _add_light(s, keep, 9), "all", INVALID, "jp_upload_scene: unknown light type"),
    "cycle": (_poke("bvh_left", lambda s: s.n_bvh_nodes, 0, 0), "all", INVALID, "jp_upload_scene: BVH is not a tree rooted at node 0 (cycle, bad child index or excessive depth)"),
    "too_deep": (_deep_tree, "all", INVALID, "jp_upload_scene: BVH height exceeds the device traversal stack (32)"),
    "leaf_range": (_poke("bvh_right", lambda s: s.n_bvh_nodes, _first_leaf, 17), "all", INVALID, "jp_upload_scene: BVH leaf range invalid (1..16 primitives per leaf)"),
    "leaf_prim_index": (_poke("bvh_prim_index", lambda s: s.n_bvh_prim_indices, 0, lambda s: s.n_primitives), "all", INVALID, "jp_upload_scene: BVH primitive index out of range"),
    "prim_in_two_leaves": (_poke("bvh_prim_index", lambda s: s.n_bvh_prim_indices, 0, lambda s: s.bvh_prim_index[1]), "all", INVALID,
                           "jp_upload_scene: every primitive must be in exactly one BVH leaf"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_keep_code_and_message(name):
    brk, mode, code, msg = REFUSALS[name]
    be, s = _cornell()
    keep = []
    brk(s, keep)
    L = jp.hip_lib()
    info = jp.JpUploadInfo(); info.struct_bytes = C.sizeof(jp.JpUploadInfo)
    assert L.jp_describe_upload(None, jp.LIGHT_SAMPLING_MODES[mode], C.byref(s), C.byref(info)) == code
    assert L.jp_last_error().decode() == msg
    be.close()


def test_describe_upload_own_arguments():
    L = jp.hip_lib()
    be, s = _cornell()
    info = jp.JpUploadInfo(); info.struct_bytes = C.sizeof(jp.JpUploadInfo)
    assert L.jp_describe_upload(None, 0, None, C.byref(info)) == INVALID and L.jp_describe_upload(None, 0, C.byref(s), None) == INVALID
    assert L.jp_describe_upload(None, 7, C.byref(s), C.byref(info)) == INVALID
    o = jp.JpOptions(); o.struct_bytes = C.sizeof(jp.JpOptions); o.traversal = 9
    assert L.jp_describe_upload(C.byref(o), 0, C.byref(s), C.byref(info)) == INVALID and "field out of range" in L.jp_last_error().decode()
    s.n_bvh_nodes = 0                                                   # no hierarchy: the trees would come from the device builders
    assert L.jp_describe_upload(None, 0, C.byref(s), C.byref(info)) == UNSUPPORTED
    # a shorter struct of the caller is truncated: nothing is written past struct_bytes
    be2, s2 = _cornell()
    full = jp.describe_upload(s2)
    short = jp.JpUploadInfo(); short.struct_bytes = 16; short.lds_bytes = -77
    assert L.jp_describe_upload(None, 0, C.byref(s2), C.byref(short)) == 0
    assert short.struct_bytes == 16 and short.trav_mode == full.trav_mode and short.stack_depth_q4 == full.stack_depth_q4 and short.lds_bytes == -77
    assert full.struct_bytes == C.sizeof(jp.JpUploadInfo)
    be.close(); be2.close()


def test_upload_info_layout_matches_header(tmp_path):
    """the ctypes mirror of JpUploadInfo has the C layout (as test_abi_struct_layout_matches_header checks the older structs)"""
    import subprocess
    src = '#include "jetpbrt_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){ printf("%zu %zu %zu %zu %d\\n", sizeof(JpUploadInfo), offsetof(JpUploadInfo, lds_bytes), offsetof(JpUploadInfo, cert_pad), offsetof(JpUploadInfo, table), JP_UPLOAD_TABLES); return 0; }'
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    I = jp.JpUploadInfo
    assert out == [C.sizeof(I), I.lds_bytes.offset, I.cert_pad.offset, I.table.offset, len(jp.UPLOAD_TABLES)]
