"""Texture-mapped materials, host side (no GPU): OBJ texture coordinates, the image readers, the flattener's JpTextures, the ctypes layout
of the new structs and the register budgets of the new kernels."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

f32 = np.float32


def _arr(p, n, dt=np.float32):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy() if n else np.zeros(0, dt)


def _scene(mesh_path=None, setup=None):
    be = scenes.HostBackend("t")
    be.camera((278, 273, 960), (0, 0, -1), (0, 1, 0), 60.0, 32, 24)
    be.envlight((0.1, 0.1, 0.1))
    if setup:
        setup(be)
    if mesh_path:
        be.mesh(mesh_path, False, False, mat=be.mat_matte((0.5, 0.5, 0.5)))
    be.preprocess()
    return be


def _tex(be):
    return be.flatten_textures().contents


# ---- 1. OBJ reader ------------------------------------------------------------------------------------------------
OBJ_UV = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.1 0.2
vt 0.3 0.4
vt 0.5 0.6
vt 0.7 0.8
vn 0 0 1
f 1 2 3
f 1/1 2/2 3/3
f 1/1/1 2/2/1 3/3/1
f 1//1 2//1 3//1
f 1/1 2/2 3/3 4/4
f -4/-4 -3/-3 -2/-2
f 1/4 2 3/2
"""


def test_obj_reader_texture_coordinates(tmp_path):
    """vt and the face forms v, v/vt, v/vt/vn, v//vn, a quad fan and negative indices flatten to the expected tri_uv
    (a vertex without vt: uv 0); transforms leave uvs alone"""
    p = str(tmp_path / "uv.obj"); open(p, "w").write(OBJ_UV)
    be = scenes.HostBackend("t")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 60.0, 8, 8)
    be.envlight((0, 0, 0))
    tex = be.texture_solid((0.5, 0.5, 0.5))
    be.mesh(p, True, True, (1, 2, 3), 2.0, be.mat_matte(tex=tex), None)
    be.preprocess()
    s = be.flatten().contents; t = _tex(be)
    assert s.n_triangles == 8 and t.n_triangles == 8 and t.n_textures == 1
    uv = _arr(t.tri_uv, 6 * 8).reshape(8, 3, 2)
    vt = np.array([(0.1, 0.2), (0.3, 0.4), (0.5, 0.6), (0.7, 0.8)], f32)
    z = np.zeros(2, f32)
    want = np.array([[z, z, z], vt[[0, 1, 2]], vt[[0, 1, 2]], [z, z, z], vt[[0, 1, 2]], vt[[0, 2, 3]], vt[[0, 1, 2]], [vt[3], z, vt[1]]], f32)
    assert np.array_equal(uv, want)
    # positions: the reference's transform (z flip, scale, offset) as before
    p0 = _arr(s.tri_p0, 24).reshape(8, 3)
    assert np.array_equal(p0[0], np.array([1, 2, 3], f32))


def test_obj_without_vt_flattens_as_before(tmp_path):
    """an OBJ without vt: the JpScene arrays equal those of the same geometry written with vt, and no textures are flattened"""
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 0.5, 1)], f32)
    f = np.array([(0, 1, 2), (0, 2, 3), (0, 1, 4)])
    a = scenes.write_obj(str(tmp_path / "a.obj"), v, f)
    b = scenes.write_obj(str(tmp_path / "b.obj"), v, f, uvs=np.random.default_rng(0).random((5, 2)))
    sa, sb = _scene(a), _scene(b)
    A, B = sa.flatten().contents, sb.flatten().contents
    assert _tex(sa).n_textures == 0
    for name in ("tri_p0", "tri_p1", "tri_p2", "tri_n"):
        assert np.array_equal(_arr(getattr(A, name), 9), _arr(getattr(B, name), 9))
    assert np.array_equal(_arr(_tex(sa).tri_uv, 18), np.zeros(18, f32))
    assert not np.array_equal(_arr(_tex(sb).tri_uv, 18), np.zeros(18, f32))


def test_obj_without_vt_flattens_to_known_arrays(tmp_path):
    """an OBJ without vt (faces v and v//vn, a quad fan, a negative index), transformed (z flip, scale, offset): the JpScene triangle arrays
    are the reference's -- positions through z flip, scale, offset, normal Normalize(Cross(p1 - p0, p2 - p0)) flipped -- computed here"""
    v = np.array([(0.5, -1.25, 3.0), (2.0, 0.75, -1.5), (1.0, 2.5, 0.25), (-0.75, 1.0, 1.5)], f32)
    txt = "".join("v %.9g %.9g %.9g\n" % tuple(map(float, p)) for p in v) + "vn 0 0 1\nf 1 2 3\nf 1//1 3//1 4//1\nf -4 -3 -2 -1\n"
    path = str(tmp_path / "novt.obj"); open(path, "w").write(txt)
    be = scenes.HostBackend("t")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 60.0, 8, 8)
    be.envlight((0, 0, 0))
    be.mesh(path, True, True, (1.5, -2.0, 0.5), 3.0, be.mat_matte((0.5, 0.5, 0.5)), None)
    be.preprocess()
    s = be.flatten().contents
    x = v.copy(); x[:, 2] = -x[:, 2]; x = (x * f32(3.0)).astype(f32); x = (x + np.array([1.5, -2.0, 0.5], f32)).astype(f32)
    tris = [(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 2, 3)]
    P = [np.array([x[t[k]] for t in tris], f32) for k in range(3)]
    a, b = (P[1] - P[0]).astype(f32), (P[2] - P[0]).astype(f32)
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1).astype(f32)
    ln = np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(f32)).astype(f32)
    n = (-(c / ln[:, None])).astype(f32)
    assert s.n_triangles == 4 and s.n_primitives == 4
    for k, name in enumerate(("tri_p0", "tri_p1", "tri_p2")):
        assert np.array_equal(_arr(getattr(s, name), 12).reshape(4, 3), P[k]), name
    assert np.array_equal(_arr(s.tri_n, 12).reshape(4, 3).view(np.uint32), n.view(np.uint32))
    assert list(_arr(s.prim_shape_type, 4, np.int32)) == [0] * 4 and list(_arr(s.prim_shape_index, 4, np.int32)) == [0, 1, 2, 3]
    assert _tex(be).n_textures == 0


# ---- 2. image readers -----------------------------------------------------------------------------------------------
def _ppm(path, img):
    h, w, _ = img.shape
    open(path, "wb").write(b"P6\n# comment\n%d %d\n255\n" % (w, h) + img.tobytes())


def _bmp(path, img, bpp=24, masks=None):
    """masks: 32-bit BI_BITFIELDS with these R, G, B masks (the pixel bytes follow them)"""
    h, w, _ = img.shape
    bpx = bpp // 8; row = (w * bpx + 3) & ~3
    data = bytearray()
    for y in range(h - 1, -1, -1):                                  # bottom-up
        r = bytearray()
        for x in range(w):
            if masks:
                px = 0x7f7f7f7f
                for c, m in enumerate(masks):
                    sh = (m & -m).bit_length() - 1
                    px = (px & ~m) | (int(img[y, x, c]) << sh)
                r += struct.pack("<I", px & 0xffffffff)
            else:
                r += bytes([img[y, x, 2], img[y, x, 1], img[y, x, 0]]) + (b"\x7f" if bpp == 32 else b"")
        data += r + b"\0" * (row - len(r))
    extra = struct.pack("<III", *masks) if masks else b""
    off = 54 + len(extra)
    hdr = struct.pack("<2sIHHI", b"BM", off + len(data), 0, 0, off) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, bpp, 3 if masks else 0, len(data), 2835, 2835, 0, 0)
    open(path, "wb").write(hdr + extra + bytes(data))


def _image_texels(path):
    be = _scene(setup=lambda b: b.sphere((0, 0, 0), 1.0, b.mat_matte(tex=b.texture_image_file(path)), None))
    t = _tex(be)
    assert t.n_textures == 1
    return be, t                                                    # (the view lives as long as the backend)


@pytest.mark.parametrize("fmt", ["ppm", "bmp24", "bmp32"])
def test_image_readers_top_row_first(tmp_path, fmt):
    """hand-built PPM (P6) and BMP (24 / 32 bit, odd width: padded rows, bottom-up) files flatten to top-row-first RGB8 texels"""
    img = np.random.default_rng(7).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    p = str(tmp_path / ("img." + fmt[:3]))
    if fmt == "ppm":
        _ppm(p, img)
    else:
        _bmp(p, img, 24 if fmt == "bmp24" else 32)
    be, t = _image_texels(p)
    assert t.tex_type[0] == jp.JP_TEXTURE_IMAGE and t.tex_width[0] == 7 and t.tex_height[0] == 5 and t.tex_offset[0] == 0
    assert t.n_texel_bytes == img.size
    assert np.array_equal(_arr(t.texels, img.size, np.uint8), img.reshape(-1))


def test_bmp_bitfields_masks(tmp_path):
    """a 32-bit BI_BITFIELDS BMP is decoded through its channel masks (here R G B in the low bytes); masks that are not whole bytes: cyan"""
    img = np.random.default_rng(8).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    p = str(tmp_path / "bf.bmp")
    _bmp(p, img, 32, masks=(0x000000ff, 0x0000ff00, 0x00ff0000))
    be, t = _image_texels(p)
    assert t.tex_type[0] == jp.JP_TEXTURE_IMAGE and np.array_equal(_arr(t.texels, img.size, np.uint8), img.reshape(-1))
    q = str(tmp_path / "bad.bmp")
    _bmp(q, img, 32, masks=(0x00000ff0, 0x0000f00f, 0x00ff0000))
    be2, t2 = _image_texels(q)
    assert t2.tex_type[0] == jp.JP_TEXTURE_SOLID and list(_arr(t2.tex_color, 3)) == [0.0, 1.0, 1.0]


@pytest.mark.parametrize("what", ["png", "missing"])
def test_unreadable_image_is_solid_cyan(tmp_path, what):
    """a PNG or a missing file: the reference's "solid cyan as a debugging aid", SOLID (0, 1, 1)"""
    p = str(tmp_path / "x.png")
    if what == "png":
        open(p, "wb").write(b"\x89PNG\r\n\x1a\n" + b"\0" * 64)
    be, t = _image_texels(p)
    assert t.tex_type[0] == jp.JP_TEXTURE_SOLID
    assert list(_arr(t.tex_color, 3)) == [0.0, 1.0, 1.0]


# ---- 3. flattener ------------------------------------------------------------------------------------------------------
def test_flattener_shares_textures_and_indexes_materials():
    """a texture shared by two materials is flattened once; mat_texture points every material at its texture (-1: none)"""
    ids = {}

    def setup(b):
        chk = b.texture_checker((1, 0, 0), (0, 0, 1))
        img = b.texture_image(np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3))
        ids["m"] = [b.mat_matte((0.2, 0.3, 0.4)), b.mat_matte(tex=chk), b.mat_mirror(tex=img), b.mat_plastic(None, (0.3, 0.3, 0.3), 0.2, False, tex=chk),
                    b.mat_glass(1.5, (1, 1, 1), (1, 1, 1))]
        for k, m in enumerate(ids["m"]):
            b.sphere((3 * k, 0, 0), 1.0, m, None)
    be = _scene(setup=setup)
    t = _tex(be)
    s = be.flatten().contents
    assert t.n_textures == 2 and t.n_materials == s.n_materials
    mt = _arr(t.mat_texture, s.n_materials, np.int32)
    m = ids["m"]
    assert mt[m[0]] == -1 and mt[m[4]] == -1 and mt[m[1]] == mt[m[3]] == 0 and mt[m[2]] == 1
    assert t.tex_type[0] == jp.JP_TEXTURE_CHECKER and t.tex_type[1] == jp.JP_TEXTURE_IMAGE
    assert list(_arr(t.tex_color, 6)) == [1, 0, 0, 0, 0, 1]
    assert t.tex_width[1] == 3 and t.tex_height[1] == 2 and t.n_texel_bytes == 18


@pytest.mark.parametrize("kind", ["glass", "metal"])
def test_flattener_refuses_texture_on_glass_or_metal(kind):
    def setup(b):
        m = b.mat_glass(1.5, (1, 1, 1), (1, 1, 1)) if kind == "glass" else b.mat_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.1, 0.1, False)
        assert b.mat_set_texture(m, b.texture_solid((1, 1, 1))) == 0
        b.sphere((0, 0, 0), 1.0, m, None)
    be = _scene(setup=setup)
    with pytest.raises(RuntimeError, match="glass or metal"):
        be.flatten()


def test_untextured_scene_has_no_textures():
    be = scenes.build_cornell(scenes.HostBackend("c"), 16, 16)
    assert _tex(be).n_textures == 0


# ---- 4. layout ------------------------------------------------------------------------------------------------------------
def test_texture_struct_layout_matches_header(H):
    src = r'''
    #include "jetpbrt_amd.h"
    #include <stdio.h>
    #include <stddef.h>
    int main(){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(JpTextures), offsetof(JpTextures, tex_offset), offsetof(JpTextures, n_texel_bytes),
                offsetof(JpTextures, texels), offsetof(JpTextures, mat_texture), offsetof(JpTextures, n_triangles), offsetof(JpTextures, tri_uv),
                sizeof(JpTextureInfo), offsetof(JpTextureInfo, texel_bytes_device), offsetof(JpTextureInfo, textured_last_render)); return 0; }'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    T, I = jp.JpTextures, jp.JpTextureInfo
    assert [int(v) for v in out] == [C.sizeof(T), T.tex_offset.offset, T.n_texel_bytes.offset, T.texels.offset, T.mat_texture.offset,
                                     T.n_triangles.offset, T.tri_uv.offset, C.sizeof(I), I.texel_bytes_device.offset, I.textured_last_render.offset]


def test_texture_symbols_exported(H):
    lib = C.CDLL(jp.HIP_LIB_PATH)
    for name in ("jp_upload_scene_textured", "jp_get_texture_info", "jp_surface"):
        assert hasattr(lib, name), name
    assert lib.jp_abi_version() == 7


# ---- 5. register budgets ---------------------------------------------------------------------------------------------------
def test_texture_kernel_register_budgets(H):
    """every k_shade_tex<...> within its k_shade counterpart's budget (168 VGPRs, 3 waves, no scratch); k_texel 8 waves, no scratch"""
    csrc = os.path.join(H.REPO, "jet-pbrt_amd", "csrc")
    subprocess.run(["make", "-s", "asm"], cwd=csrc, check=True)
    out = subprocess.run([sys.executable, os.path.join(H.REPO, "tools", "resource_table.py")], stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), scratch=int(m.group(5)), waves=int(m.group(6)))
    tex = [n for n in rows if n.startswith("k_shade_tex<")]
    assert len(tex) == 10
    for n in tex:
        base = rows[n.replace("k_shade_tex<", "k_shade<")]
        r = rows[n]
        assert r["scratch"] == 0 and r["vgpr"] <= max(168, base["vgpr"]) and r["waves"] >= min(3, base["waves"]), (n, r, base)
    assert rows["k_texel"]["scratch"] == 0 and rows["k_texel"]["waves"] == 8, rows["k_texel"]
