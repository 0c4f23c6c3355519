"""CPU suite, part 3: host-side logic (scene description, OBJ ingest, BVH builder, flattener) and the C-ABI
library: it must load without a GPU and export every symbol include/jetpbrt_amd.h declares.  No compute call
is made here."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest


def _flat(H, name, W=32, Hh=24):
    hb = H.SCENES[name](H.scenes.HostBackend(name), W, Hh)
    return hb, hb.flatten().contents


def test_abi_exports_every_declared_symbol(H):
    hdr = open(os.path.join(H.REPO, "include", "jetpbrt_amd.h")).read()
    names = sorted(set(re.findall(r"\b(jp_[a-z_]+)\s*\(", hdr)))
    assert {"jp_create_context", "jp_upload_scene", "jp_render", "jp_render_device", "jp_get_counters", "jp_trace", "jp_occluded", "jp_last_error"} <= set(names)
    lib = C.CDLL(H.jp.HIP_LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "libjetpbrt_amd.so does not export %s" % n
    assert lib.jp_abi_version() == 7 == H.jp.JP_ABI_VERSION
    assert {"jp_set_options", "jp_get_options"} <= set(names)          # ABI 7: the switches by value


def test_abi_struct_layout_matches_header(H):
    """the ctypes mirrors must have the C sizes (x86-64 SysV): guards against drift between header and bindings."""
    src = r'''
    #include "jetpbrt_amd.h"
    #include <stdio.h>
    #include <stddef.h>
    int main(){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(JpScene), sizeof(JpRenderParams), sizeof(JpCounters), sizeof(JpCamera),
                offsetof(JpScene, bvh_prim_index), offsetof(JpScene, world_radius), sizeof(JpBuildInfo), offsetof(JpBuildInfo, device_build_ms),
                sizeof(JpOptions), offsetof(JpOptions, max_slots), offsetof(JpOptions, cert_slack), offsetof(JpOptions, reserved)); return 0; }'''
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    jp = H.jp
    assert [int(v) for v in out] == [C.sizeof(jp.JpScene), C.sizeof(jp.JpRenderParams), C.sizeof(jp.JpCounters), C.sizeof(jp.JpCamera),
                                     jp.JpScene.bvh_prim_index.offset, jp.JpScene.world_radius.offset,
                                     C.sizeof(jp.JpBuildInfo), jp.JpBuildInfo.device_build_ms.offset,
                                     C.sizeof(jp.JpOptions), jp.JpOptions.max_slots.offset, jp.JpOptions.cert_slack.offset, jp.JpOptions.reserved.offset]


def test_device_build_flag_flattens_without_a_hierarchy(H):
    """FScene::deviceBuild: Preprocess() skips the host tree and the flattened scene says so (n_bvh_nodes == 0);
    everything else is identical to the host-built flattening"""
    hb = H.scenes.HostBackend("dev"); hb.set_device_build(True)
    H.SCENES["misc"](hb, 32, 24)
    a = hb.flatten().contents
    hb2, b = _flat(H, "misc")
    assert a.n_bvh_nodes == 0 and b.n_bvh_nodes > 0
    assert a.n_primitives == b.n_primitives and a.n_lights == b.n_lights and a.world_radius == b.world_radius
    n = a.n_primitives
    for f in ("prim_shape_type", "prim_shape_index", "prim_material", "prim_light"):
        assert np.array_equal(np.ctypeslib.as_array(getattr(a, f), (n,)), np.ctypeslib.as_array(getattr(b, f), (n,)))


def test_library_reads_the_environment_in_one_place_only(H):
    """ABI 7: the kernel library's switches are JpOptions; the environment is read once per context by ONE table-driven loader
    (round 3 had 42 getenv call sites that were consulted at upload / render time)"""
    csrc = os.path.join(H.REPO, "jet-pbrt_amd", "csrc")
    n = 0
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            n += len(re.findall(r"\bgetenv\s*\(", open(os.path.join(csrc, f), errors="ignore").read()))
    assert n == 1, n
    hdr = open(os.path.join(H.REPO, "include", "jetpbrt_amd.h")).read()
    fields = re.findall(r"^\s+(?:int32_t|int64_t|float)\s+([a-z_0-9, ]+);", hdr[hdr.index("typedef struct JpOptions"):hdr.index("} JpOptions;")], re.M)
    names = [x.strip() for f in fields for x in f.split(",")]
    mirror = [n for n, _ in H.jp.JpOptions._fields_]
    assert [n.split("[")[0] for n in names] + ["reserved"] == mirror or [n.split("[")[0] for n in names] == mirror, (names, mirror)


def test_product_does_not_reference_oracle(H):
    """the shipped path must never route through the oracle or the reference build"""
    pkg = os.path.join(H.REPO, "jet-pbrt_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".cc", ".hip", "Makefile")):
                txt = open(os.path.join(root, f), errors="ignore").read()
                assert "libjp_oracle" not in txt and "libjp_ref" not in txt and "pt_oracle" not in txt, os.path.join(root, f)
                assert not re.search(r"^\s*(from|import)\s+.*\b(oracle|harness)\b", txt, re.M), os.path.join(root, f)
    import subprocess
    for so in (H.jp.HIP_LIB_PATH, H.jp.HOST_LIB_PATH):
        needed = subprocess.run(["readelf", "-d", so], stdout=subprocess.PIPE, text=True).stdout
        assert "jp_oracle" not in needed and "jp_ref" not in needed


@pytest.mark.parametrize("name", ["cornell", "bunny_small", "misc"])
def test_flatten_and_bvh_invariants(H, name):
    hb, s = _flat(H, name)
    n = s.n_primitives
    assert n == hb.num_primitives() and s.n_lights == hb.num_lights()
    st = np.ctypeslib.as_array(s.prim_shape_type, (n,)); si = np.ctypeslib.as_array(s.prim_shape_index, (n,))
    for kind, cnt in ((0, s.n_triangles), (1, s.n_rectangles), (2, s.n_spheres)):
        idx = np.sort(si[st == kind])
        assert np.array_equal(idx, np.arange(cnt))                       # every shape referenced exactly once
    left = np.ctypeslib.as_array(s.bvh_left, (s.n_bvh_nodes,)); right = np.ctypeslib.as_array(s.bvh_right, (s.n_bvh_nodes,))
    bounds = np.ctypeslib.as_array(s.bvh_bounds, (s.n_bvh_nodes, 6)); pidx = np.ctypeslib.as_array(s.bvh_prim_index, (s.n_bvh_prim_indices,))
    assert np.array_equal(np.sort(pidx), np.arange(n))                   # every primitive in exactly one leaf
    seen = np.zeros(s.n_bvh_nodes, bool)
    def walk(i, depth):
        assert not seen[i]; seen[i] = True
        if left[i] < 0:
            assert 1 <= right[i] <= 4
            return depth
        for c in (left[i], right[i]):
            assert (bounds[c, :3] >= bounds[i, :3] - 1e-4).all() and (bounds[c, 3:] <= bounds[i, 3:] + 1e-4).all()   # children inside parent
        return max(walk(left[i], depth + 1), walk(right[i], depth + 1))
    h = walk(0, 0)
    assert seen.all() and h < 32
    # light table: env light first, then one area light per emitting shape, each pointing at a primitive that points back
    lt = np.ctypeslib.as_array(s.light_type, (s.n_lights,)); lp = np.ctypeslib.as_array(s.light_prim, (s.n_lights,)); pl = np.ctypeslib.as_array(s.prim_light, (n,))
    assert lt[0] == 0 and lp[0] == -1
    for li in range(1, s.n_lights):
        assert lt[li] == 1 and pl[lp[li]] == li
    assert s.world_radius > 100


def test_camera_and_world_radius_match_reference_kats(H, kat):
    """FCamera ctor (camera.h:36-49) and FEnvironmentLight::Preprocess (light.cc:26-33) restated on the host:
    camera rays generated from the flattened camera equal the reference's GenerateRay KATs bit for bit (through
    the oracle's 3-line camera function), and env-light samples (which embed worldRadius) equal the light KATs --
    both covered in test_oracle_golden; here: plain sanity of the values."""
    hb, s = _flat(H, "cornell", 48, 48)
    assert tuple(s.camera.pos) == (278.0, 273.0, 960.0) and tuple(s.camera.front) == (0.0, 0.0, -1.0)
    assert abs(s.camera.up[1] - np.tan(np.radians(30.0))) < 1e-6 and s.camera.res_x == 48.0


def test_obj_reader_variants(H, tmp_path):
    """own OBJ reader: v/vt/vn index forms, negative indices, polygon fans, comments; transform order of
    shape.cc:48-61 (z flip, scale, offset)."""
    p = tmp_path / "m.obj"
    p.write_text("# c\no m\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0.5\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\nf 1//1 3//1 4//1\nf -4 -3 -2 -1\n")
    be = H.scenes.HostBackend("obj")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 60.0, 8, 8)
    be.envlight((0, 0, 0))
    m = be.mat_matte((0.5, 0.5, 0.5))
    ntri = be.mesh(str(p), False, True, (10, 20, 30), 2.0, m, None)
    assert ntri == 4                                                       # 2 triangles + a quad as a 2-triangle fan
    be.preprocess()
    s = be.flatten().contents
    p2 = np.ctypeslib.as_array(s.tri_p2, (4, 3))
    assert np.allclose(p2[1], [0 * 2 + 10, 1 * 2 + 20, -0.5 * 2 + 30])    # vertex 4: z flipped, scaled, offset
    n0 = np.ctypeslib.as_array(s.tri_n, (4, 3))[0]
    assert np.allclose(np.abs(n0), [0, 0, 1])


def test_missing_mesh_and_flatten_errors(H, tmp_path):
    be = H.scenes.HostBackend("err")
    be.camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 60.0, 8, 8)
    m = be.mat_matte((0.5, 0.5, 0.5))
    assert be.mesh(str(tmp_path / "nope.obj"), False, False, (0, 0, 0), 1.0, m, None) == 0     # reference convention: prints, empty mesh
    assert not H.jp.host_lib().jp_host_flatten(be.h)                                             # not preprocessed
    assert b"Preprocess" in H.jp.host_lib().jp_host_last_error(be.h)


def test_create_context_without_gpu_fails_loudly(H):
    """on a machine without a GPU the product must refuse, not fall back"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(H.jp.JetPbrtError) as e:
        H.jp.Context(0)
    assert "no HIP device" in str(e.value) or "status -2" in str(e.value)


def test_film_writers(H, tmp_path):
    """FFilm::SaveAsImage (film.cc:11-188 behaviour, format rules applied properly): PPM P3 with decimal samples, BMP with
    4-byte row padding for a width with width*3 % 4 != 0, Radiance HDR; gamma_encoding = uint8(pow(clamp01(x), 1/2.2) * 255)."""
    W, Hh = 5, 3                                   # 15 bytes per row -> padded to 16
    rng = np.random.default_rng(1)
    rgb = rng.uniform(-0.2, 1.3, (Hh, W, 3)).astype(np.float32); rgb[0, 0] = (0, 0, 0); rgb[1, 2] = (1e-35, 0, 0)
    rgb[..., 1:] = np.abs(rgb[..., 1:]); rgb[:, 1:, 0] = np.abs(rgb[:, 1:, 0]); rgb[2, 0, 0] = -0.1     # one negative channel: clamps to 0 in the 8-bit formats
    L = H.jp.host_lib()
    base = str(tmp_path / "img")
    for t in (0, 1, 2):
        assert L.jp_host_save_image(rgb.ctypes.data, W, Hh, base.encode(), t) == 1
    enc = (np.power(np.clip(rgb.astype(np.float32), 0, 1), np.float32(1 / 2.2)).astype(np.float64) * 255.0).astype(np.uint8)
    tok = open(base + ".ppm").read().split()
    assert tok[:4] == ["P3", str(W), str(Hh), "255"]
    ppm = np.array(tok[4:], int).reshape(Hh, W, 3)
    assert np.abs(ppm - enc.astype(int)).max() <= 1          # pow() last-bit differences only
    raw = open(base + ".bmp", "rb").read()
    assert raw[:2] == b"BM" and int.from_bytes(raw[2:6], "little") == len(raw) == 54 + 16 * Hh
    assert int.from_bytes(raw[18:22], "little") == W and int.from_bytes(raw[22:26], "little") == Hh and int.from_bytes(raw[28:30], "little") == 24
    body = np.frombuffer(raw[54:], np.uint8).reshape(Hh, 16)[::-1, : 3 * W].reshape(Hh, W, 3)[..., ::-1]   # bottom-up, BGR
    assert np.array_equal(body, ppm.astype(np.uint8))
    hdr = open(base + ".hdr", "rb").read()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 3 +X 5\n"
    assert hdr.startswith(head) and len(hdr) == len(head) + 4 * W * Hh
    px = np.frombuffer(hdr[len(head):], np.uint8).reshape(Hh, W, 4)
    assert tuple(px[0, 0]) == (0, 0, 0, 0) and tuple(px[1, 2]) == (0, 0, 0, 0)
    e = px[..., 3].astype(int) - 128 - 8
    dec = px[..., :3].astype(np.float64) * np.exp2(e)[..., None]
    pos = np.clip(rgb, 0, None)
    live = (rgb.max(-1) >= 1e-32) & (rgb.min(-1) >= 0)
    assert np.abs(dec[live] - pos[live]).max() <= rgb.max() / 128 + 1e-6


def test_cli_usage_and_no_gpu_behaviour(H, tmp_path):
    """`jetpbrt` mirrors main.cc:113-163: no arguments -> usage line, exit 0; without a GPU it must fail loudly and write nothing"""
    import subprocess
    r = subprocess.run([H.jp.CLI_PATH], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "sceneid" in r.stderr
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    root = H.scenes.export_reference_layout(str(tmp_path / "scene"), 12, 8)
    r = subprocess.run([H.jp.CLI_PATH, "0", "1", "16", "16", "--assets", root, "--out", str(tmp_path / "o")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 3 and not (tmp_path / "o.bmp").exists()
    assert "no HIP device" in r.stderr or "not available" in r.stderr


def test_reference_tree_builder_reproduces_the_reference_topology(H):
    """FScene::referenceTree: the host rebuilds the reference's own BVH (glibc rand() sequence from seed 1 restated, same
    std::sort over the same ranges).  Node for node equal to the oracle's tree, which is pinned to the compiled reference."""
    for name, extra in (("bunny_small", None), ("misc", None)):
        hb = H.scenes.HostBackend(name); hb.set_reference_tree(True)
        H.SCENES[name](hb, 32, 24)
        s = hb.flatten().contents
        assert s.bvh_reference_semantics == 1 and s.n_bvh_nodes > 0
        nn = s.n_bvh_nodes
        B = np.ctypeslib.as_array(s.bvh_bounds, (nn * 6,)).reshape(nn, 6); L = np.ctypeslib.as_array(s.bvh_left, (nn,)); R = np.ctypeslib.as_array(s.bvh_right, (nn,))
        P = np.ctypeslib.as_array(s.bvh_prim_index, (s.n_bvh_prim_indices,))
        boxes, kind, order = [], [], []

        def walk(n):
            boxes.append(B[n]);
            if L[n] < 0:
                first = -L[n] - 1; kind.append(int(R[n])); order.extend(int(v) for v in P[first:first + R[n]]); return
            kind.append(-1); walk(L[n]); walk(R[n])
        import sys
        sys.setrecursionlimit(10000)
        walk(0)
        H.libc_srand(1)                                           # the reference process' default rand() state
        Lo = H.oracle_lib(); oh = H.oracle_scene(Lo, hb.flatten())
        ob = np.zeros((4 * s.n_primitives + 8, 6), np.float32); ok = np.zeros(4 * s.n_primitives + 8, np.int32); oo = np.zeros(s.n_primitives, np.int32)
        n = Lo.jp_oracle_tree_dump(oh, H.ptr(ob), H.ptr(ok), H.ptr(oo), len(ok))
        Lo.jp_oracle_scene_free(oh)
        assert n == len(kind), (n, len(kind))
        assert np.array_equal(ok[:n], np.array(kind, np.int32)) and np.array_equal(oo, np.array(order, np.int32))
        assert np.array_equal(ob[:n].view(np.uint32), np.array(boxes, np.float32).view(np.uint32))


def test_certified_walk_flag_reaches_the_scene_record(H, monkeypatch):
    """FScene::certifiedWalk: JpScene.bvh_reference_semantics 2 with the same (reference) tree as 1; also from the environment"""
    def flat(**kw):
        hb = H.scenes.HostBackend("misc")
        if kw: hb.set_reference_tree(True, **kw)
        H.SCENES["misc"](hb, 32, 24)
        s = hb.flatten().contents
        nn = s.n_bvh_nodes
        return s.bvh_reference_semantics, np.ctypeslib.as_array(s.bvh_bounds, (nn * 6,)).copy(), np.ctypeslib.as_array(s.bvh_left, (nn,)).copy()
    m1, b1, l1 = flat(certified=False)
    m2, b2, l2_ = flat(certified=True)
    assert (m1, m2) == (1, 2) and np.array_equal(b1, b2) and np.array_equal(l1, l2_)
    monkeypatch.setenv("JETPBRT_REFERENCE_TREE", "2")
    m3, b3, l3 = flat()
    assert m3 == 2 and np.array_equal(b1, b3)
    monkeypatch.setenv("JETPBRT_REFERENCE_TREE", "1")
    assert flat()[0] == 1


def test_libm_sincosf_transcription_matches_this_host(H):
    """the device reproduces the host libm's sinf / cosf / sincosf from a transcription of glibc's algorithm (jp_shading.h
    sincosf_libm); the library checks that transcription against the running libm on 200,000 arguments -- on this image
    (glibc 2.35) it must match, otherwise the bit-identical film tests would silently fall back to a tolerance"""
    lib = C.CDLL(H.jp.HIP_LIB_PATH)
    assert lib.jp_probe_libm_sincosf() in (1, 2)


def test_film_writers_equal_the_reference_writers_byte_for_byte(H, tmp_path):
    """golden BMP / HDR bytes written by the reference's own film.cc (tests/golden/make_golden_film_io.py; a
    width whose rows need no padding, pixels >= 1e-32 -- where the reference's writers are correct) against this host's writers,
    and gamma_encoding (film.h:24) around every step of the 8-bit curve against the host mirror AND against the threshold table the
    device tone map uses (jp_gamma_thresholds: byte = number of thresholds <= x)."""
    g = np.load(os.path.join(H.GOLDEN, "film_io.npz"))
    film = np.ascontiguousarray(g["film"]); Hh, W = film.shape[:2]
    L = H.jp.host_lib()
    base = str(tmp_path / "img")
    for t, ext in ((1, "bmp"), (2, "hdr")):
        assert L.jp_host_save_image(film.ctypes.data, W, Hh, base.encode(), t) == 1
        mine = np.frombuffer(open(base + "." + ext, "rb").read(), np.uint8)
        assert mine.size == g["file_" + ext].size and np.array_equal(mine, g["file_" + ext]), ext
    x = np.ascontiguousarray(g["gamma_x"]); want = g["gamma_y"]
    got = np.zeros(x.size, np.uint8)
    L.jp_host_gamma_encode(x.ctypes.data, x.size, got.ctypes.data)
    assert np.array_equal(got, want)
    thr = np.zeros(255, np.float32)
    assert C.CDLL(H.jp.HIP_LIB_PATH).jp_gamma_thresholds(thr.ctypes.data_as(C.c_void_p)) == 0
    assert (np.diff(thr) >= 0).all() and thr[0] > 0 and thr[-1] <= 1.0
    table = np.searchsorted(thr, np.clip(x, 0, 1), side="right").astype(np.uint8)        # what k_tonemap8 computes
    assert np.array_equal(table, want)
    # a larger random set against the reference's bytes for it (their SHA-256: tests/golden/make_golden_vs_reference.py)
    xr = gamma_sample()
    want = str(np.load(os.path.join(H.GOLDEN, "vs_reference.npz"))["gamma_sha256"])
    assert hashlib.sha256(np.searchsorted(thr, xr, side="right").astype(np.uint8).tobytes()).hexdigest() == want


def gamma_sample():
    rng = np.random.default_rng(5)
    return np.concatenate([rng.random(200000), rng.random(50000) ** 8]).astype(np.float32)


def test_kernel_register_budgets(H, tmp_path):
    """Occupancy cliffs, checked at build time (no GPU): hipcc's resource-usage remarks for the kernels of the benchmark configurations.
    k_shade sits at 167 VGPRs with the material sort -- 168 is the last count that still fits 3 waves per SIMD (512 / 168), and a build
    that crossed it lost 25 % on configs[2] during round 2; the traversal kernels must keep 8 waves per SIMD (<= 64 VGPRs), the refill
    kernels too.  No kernel may spill."""
    import subprocess
    csrc = os.path.join(H.REPO, "jet-pbrt_amd", "csrc")
    subprocess.run(["make", "-s", "asm"], cwd=csrc, check=True)
    out = subprocess.run([sys.executable, os.path.join(H.REPO, "tools", "resource_table.py")], stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1).strip()] = dict(vgpr=int(m.group(2)), scratch=int(m.group(5)), waves=int(m.group(6)))
    assert len(rows) > 40
    for name in ("k_shade<true, true, true, true>", "k_shade<true, true, true, false>", "k_shade<true, false, true, true>"):
        assert rows[name]["vgpr"] <= 168 and rows[name]["waves"] >= 3 and rows[name]["scratch"] == 0, (name, rows[name])
    for name in ("k_extend<2>", "k_extend<0>", "k_extend_persist<0, 16, true>", "k_shadow_persist<3, 16, true>", "k_extend_persist<5, 16, false>",
                 "k_extend_persist<4, 16, true>", "k_shadow_persist<4, 16, true>"):
        assert rows[name]["vgpr"] <= 64 and rows[name]["waves"] == 8 and rows[name]["scratch"] == 0, (name, rows[name])
    # the certified walk (the 4-wide walk + certificate + the verbatim walk behind it): round 4 compiles it for 8 waves per SIMD too -- measured +4 % over 7 waves
    # (profiles/r04e_certified_waves.txt); the shadow kernel then keeps ONE 64-bit value in scratch, the pointer into the global stack-spill area, reloaded only on
    # the spill path that almost no ray reaches
    for name in ("k_extend_persist<6, 16, true>", "k_shadow_persist<6, 16, true>"):
        assert rows[name]["vgpr"] <= 64 and rows[name]["waves"] == 8 and rows[name]["scratch"] <= 8, (name, rows[name])
    assert rows["k_shadow<2>"]["waves"] >= 6
    # (k_path, the opt-in fused schedule: register allocation aimed at 3 waves per SIMD, a few phase-level values spill outside its inner loops)
    assert all(r["waves"] >= 3 for n, r in rows.items() if n.startswith("k_path"))
    spills = [n for n, r in rows.items() if r["scratch"] and not n.startswith(("k_other", "k_wide_level", "k_path", "k_shadow_persist<6", "k_extend_persist<6"))]
    assert not spills, spills


def test_gamma_threshold_table_is_exact_for_every_float(H):
    """jp_render_rgb8's tone map counts host-derived thresholds <= x; the table is found by binary search, which assumes the host's
    powf-based gamma_encoding (film.h:24) never steps down.  Sweep EVERY fp32 bit pattern of [0, 1] (1,065,353,217 values) through
    both: zero differences, so the device bytes equal the host's for every input, not only for the sampled ones"""
    lib = C.CDLL(H.jp.HIP_LIB_PATH)
    lib.jp_gamma_sweep.restype = C.c_longlong
    assert lib.jp_gamma_sweep(len(os.sched_getaffinity(0))) == 0
