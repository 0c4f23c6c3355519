"""Environment maps on the host (INTEGRATION.md "Environment maps"): struct layout, the table builder against the float64 restatement of
tests/envmap_ref.py, its refusals, the image readers behind FEnvironmentMap, and the register budgets of the k_shade_env kernels.  No GPU needed."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import envmap_ref as E
from test_light_table_host import check_table

f32 = np.float32
TINT = (0.5, 1.0, 0.75)


# ---- struct layout -----------------------------------------------------------------------------------------------------------------
def test_struct_layout(H):
    src = r'''#include <stdio.h>
    #include <stddef.h>
    #include "jetpbrt_amd.h"
    int main(){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(JpEnvMap), offsetof(JpEnvMap, width), offsetof(JpEnvMap, up_axis), offsetof(JpEnvMap, importance),
                offsetof(JpEnvMap, rgb), sizeof(JpEnvInfo), offsetof(JpEnvInfo, importance), offsetof(JpEnvInfo, n_selectable), offsetof(JpEnvInfo, total_weight),
                offsetof(JpEnvInfo, mean_sum), offsetof(JpEnvInfo, mapped_last_render), offsetof(JpEnvInfo, table_bytes_device), (size_t)JP_ABI_VERSION); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    M, I = jp.JpEnvMap, jp.JpEnvInfo
    assert got == [C.sizeof(M), M.width.offset, M.up_axis.offset, M.importance.offset, M.rgb.offset, C.sizeof(I), I.importance.offset, I.n_selectable.offset,
                   I.total_weight.offset, I.mean_sum.offset, I.mapped_last_render.offset, I.table_bytes_device.offset, 7]
    lib = C.CDLL(jp.HIP_LIB_PATH)
    for name in ("jp_set_environment_map", "jp_get_env_info", "jp_env_lookup", "jp_env_sample", "jp_build_environment_table"):
        assert hasattr(lib, name), name
    assert lib.jp_abi_version() == 7


# ---- table builder ------------------------------------------------------------------------------------------------------------------
def _odd_map():
    rng = np.random.default_rng(11)
    m = rng.uniform(0.0, 3.0, (3, 5, 3)).astype(f32)
    m[1, 2] = 0.0
    return m


@pytest.mark.parametrize("name", ["bright_16x8", "odd_5x3"])
@pytest.mark.parametrize("importance", [0, -1])
def test_table_builder_is_the_definition(name, importance):
    rgb = E.bright_map() if name == "bright_16x8" else _odd_map()
    Hh, W = rgb.shape[:2]
    t = jp.build_environment_table(rgb, TINT, importance=importance)
    w_ref = E.weights(rgb, TINT, importance)
    assert t["weight"].shape == (W * Hh,) and np.allclose(t["weight"], w_ref, rtol=1e-12, atol=0.0)        # numpy's cos may differ from libm's in the last place
    w = t["weight"]
    assert t["total"] == E.total(w)
    q, alias, _ = jp.build_light_table(w)
    assert np.array_equal(t["q"], q) and np.array_equal(t["alias"], alias)                                # exactly what build_light_table makes of w
    check_table(w, t["q"], t["alias"], (w / E.total(w)).astype(f32))
    # texel records and row cosines: the fp32 roundings of the restatement's doubles, recomputed from the returned weights
    assert np.array_equal(t["texel"][:, :3].view(np.uint32), E.tinted(rgb, TINT).reshape(-1, 3).view(np.uint32))
    pdf = E.texel_pdf(w, W, Hh)
    got = t["texel"][:, 3]
    assert np.array_equal(got, pdf.astype(f32))
    ct, cb = E.row_cos(Hh)
    assert np.array_equal(t["row_cos"][:, 0], ct.astype(f32)) and np.array_equal(t["row_cos"][:, 1], cb.astype(f32))
    assert np.isclose(t["mean_sum"], E.mean_sum(rgb, TINT), rtol=1e-12)
    black = w == 0
    if importance == 0:
        assert black.sum() == (W if name == "bright_16x8" else 1)
        assert (t["q"][black] == 0).all() and not black[t["alias"][t["q"] < 1]].any()                     # a black texel is in no bin's reach
        assert (got[black] == 0).all()
    else:
        assert not black.any()
        pmf = w / E.total(w)
        assert np.allclose(pmf, np.repeat(E.omega(W, Hh), W) / (4 * np.pi), rtol=1e-12)                   # uniform solid angle
        assert np.allclose(got, 1.0 / (4 * np.pi), rtol=1e-6)


def test_constant_map_is_the_constant_light():
    """every texel 1: mean_sum is the tint's sum, so the map light's table weight is today's environment light's"""
    t = jp.build_environment_table(np.ones((4, 8, 3), f32), (0.3, 0.3, 0.3))
    s = (float(f32(0.3)) + float(f32(0.3))) + float(f32(0.3))
    assert np.isclose(t["mean_sum"], s, rtol=1e-12)
    z = jp.build_environment_table(np.zeros((4, 8, 3), f32))
    assert z["total"] == 0.0 and z["mean_sum"] == 0.0 and not z["texel"].any() and (z["alias"] == np.arange(32)).all()


def _refused(m, text, tint=(1, 1, 1)):
    with pytest.raises(jp.JetPbrtError) as e:
        jp.build_environment_table(m, tint)
    assert "status -1" in str(e.value) and text in str(e.value), str(e.value)


def test_refusals():
    ok = np.ones((2, 4, 3), f32)
    for w, h in ((0, 2), (2, 0), (4097, 2), (2, 4097)):
        m = jp.env_map(ok); m.width, m.height = w, h
        _refused(m, "size out of range")
    for bad in (np.nan, np.inf, -0.5):
        a = ok.copy(); a[1, 2, 1] = bad
        _refused(a, "negative or not finite")
    m = jp.env_map(ok); m.rgb = None
    _refused(m, "null rgb")
    m = jp.env_map(ok); m.struct_bytes = 8
    _refused(m, "struct_bytes")
    m = jp.env_map(ok); m.up_axis = 2
    _refused(m, "up_axis")
    m = jp.env_map(ok); m.importance = 3
    _refused(m, "importance")
    _refused(ok, "tint", tint=(1, -1, 1))
    assert jp.hip_lib().jp_build_environment_table(None, None, None, None, None, None, None, None, None) == -1


# ---- readers ------------------------------------------------------------------------------------------------------------------------
def _read(path, up="y"):
    be = scenes.HostBackend("envmap_reader")
    be.envmap(str(path), up)
    m = be.flatten_envmap()
    a = np.ctypeslib.as_array(m.rgb, shape=(m.height, m.width, 3)).copy()
    assert m.up_axis == jp.ENV_UP_AXES[up] and m.importance == 0
    be.close()
    return a


def _refused_file(path):
    be = scenes.HostBackend("envmap_reader")
    with pytest.raises(RuntimeError) as e:
        be.envmap(str(path))
    assert os.path.basename(str(path)) in str(e.value)
    assert be.flatten_envmap() is None
    be.close()


def _pfm(path, a, little=True):
    a = np.asarray(a, f32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n%s\n" % (a.shape[1], a.shape[0], b"-1.0" if little else b"1.0"))
        f.write(a[::-1].astype("<f4" if little else ">f4").tobytes())


def test_readers(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.uniform(0.0, 20.0, (3, 5, 3)).astype(f32)
    _pfm(tmp_path / "a.pfm", a)
    assert np.array_equal(_read(tmp_path / "a.pfm"), a)
    _pfm(tmp_path / "b.pfm", a, little=False)
    assert np.array_equal(_read(tmp_path / "b.pfm", "z"), a)
    # a film written by WriteHDR reads back within the RGBE quantum: 2^(e - 128) / 256 with 2^(e - 129) <= max channel < 2^(e - 128)
    film = rng.uniform(0.0, 1.0, (4, 6, 3)).astype(f32) * np.array([4.0, 1.0, 0.01], f32)
    film[0, 0] = 0.0
    assert jp.host_lib().jp_host_save_image(film.ctypes.data_as(C.c_void_p), 6, 4, str(tmp_path / "f").encode(), 2) == 1
    back = _read(tmp_path / "f.hdr")
    quantum = 2.0 ** np.ceil(np.log2(np.maximum(film.max(-1, keepdims=True), 1e-30)) + 1e-9) / 256.0
    assert back.shape == film.shape and (np.abs(back - film) <= quantum).all() and (back <= film).all() and not back[0, 0].any()
    assert np.abs(back - film).max() > 0
    # 8-bit formats: 1/255 per step
    img = rng.integers(0, 256, (2, 3, 3), dtype=np.uint8)
    with open(tmp_path / "c.ppm", "wb") as f:
        f.write(b"P6\n3 2\n255\n" + img.tobytes())
    assert np.array_equal(_read(tmp_path / "c.ppm"), img.astype(f32) / f32(255))
    # refused: truncated files of every format, a negative value, something else
    raw = open(tmp_path / "a.pfm", "rb").read()
    open(tmp_path / "t.pfm", "wb").write(raw[:-5]); _refused_file(tmp_path / "t.pfm")
    open(tmp_path / "t2.pfm", "wb").write(raw[:4]); _refused_file(tmp_path / "t2.pfm")
    raw = open(tmp_path / "f.hdr", "rb").read()
    open(tmp_path / "t.hdr", "wb").write(raw[:-1]); _refused_file(tmp_path / "t.hdr")
    open(tmp_path / "t2.hdr", "wb").write(raw[:20]); _refused_file(tmp_path / "t2.hdr")
    raw = open(tmp_path / "c.ppm", "rb").read()
    open(tmp_path / "t.ppm", "wb").write(raw[:-1]); _refused_file(tmp_path / "t.ppm")
    neg = a.copy(); neg[1, 1, 1] = -1.0
    _pfm(tmp_path / "n.pfm", neg); _refused_file(tmp_path / "n.pfm")
    open(tmp_path / "x.png", "wb").write(b"\x89PNG\r\n\x1a\n" + bytes(64)); _refused_file(tmp_path / "x.png")
    _refused_file(tmp_path / "missing.pfm")
    # from memory, and cleared
    be = scenes.HostBackend("envmap_memory")
    be.envmap(a, "z", importance=-1)
    m = be.flatten_envmap()
    assert (m.width, m.height, m.up_axis, m.importance) == (5, 3, 0, -1) and np.array_equal(np.ctypeslib.as_array(m.rgb, shape=(3, 5, 3)), a)
    be.envmap(None)
    assert be.flatten_envmap() is None
    be.close()


# ---- register budgets ------------------------------------------------------------------------------------------------------------------
def test_env_kernel_register_budgets(H):
    """every k_shade_env* instance within its k_shade_pick* counterpart's class: no scratch, >= 3 waves per SIMD, VGPRs <= max(168, the counterpart's)"""
    csrc = os.path.join(H.REPO, "jet-pbrt_amd", "csrc")
    subprocess.run(["make", "-s", "asm"], cwd=csrc, check=True)
    out = subprocess.run([sys.executable, os.path.join(H.REPO, "tools", "resource_table.py")], stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), scratch=int(m.group(5)), waves=int(m.group(6)))
    env = [n for n in rows if n.startswith("k_shade_env<") or n.startswith("k_shade_env_tex<")]
    assert len(env) == 20
    for n in env:
        base = rows[n.replace("k_shade_env", "k_shade_pick")]
        r = rows[n]
        assert r["scratch"] == 0 and r["waves"] >= 3 and r["vgpr"] <= max(168, base["vgpr"]), (n, r, base)
    assert rows["k_env_probe"]["scratch"] == 0
