"""Guides and denoising, host side (no GPU): the exported symbols and the ABI version, the ctypes layout of the new structs against a compiled C
probe, the host header's new film requests, the command line's new flags, and the numpy restatement of the filter's definition that the GPU tests
hold the device to (it must run without a floating-point exception on their inputs)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import jet_pbrt_amd as jp
import denoise_ref as R

f32 = np.float32


def test_denoise_symbols_exported_and_abi_unchanged(H):
    lib = jp.hip_lib()
    for name in ("jp_render_guides", "jp_render_guides_device", "jp_denoise", "jp_denoise_device", "jp_get_denoise_info", "jp_render_denoised"):
        assert hasattr(lib, name), name
    assert lib.jp_abi_version() == 7 and jp.JP_ABI_VERSION == 7
    assert hasattr(jp.host_lib(), "jp_host_render_denoised")
    for name in ("render_guides", "render_guides_device", "denoise", "denoise_device", "denoise_info"):
        assert callable(getattr(jp.Context, name)), name


def test_denoise_struct_layouts_match_the_header(H):
    src = r'''
    #include "jetpbrt_amd.h"
    #include <stdio.h>
    #include <stddef.h>
    int main(){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(JpDenoiseParams), offsetof(JpDenoiseParams, width), offsetof(JpDenoiseParams, height),
                offsetof(JpDenoiseParams, iterations), offsetof(JpDenoiseParams, sigma_color), offsetof(JpDenoiseParams, sigma_normal), offsetof(JpDenoiseParams, sigma_depth),
                offsetof(JpDenoiseParams, demodulate), sizeof(JpDenoiseInfo), offsetof(JpDenoiseInfo, sigma_color), offsetof(JpDenoiseInfo, demodulated),
                offsetof(JpDenoiseInfo, guide_spp), offsetof(JpDenoiseInfo, denoise_ms), offsetof(JpDenoiseInfo, guides_ms)); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    P, I = jp.JpDenoiseParams, jp.JpDenoiseInfo
    assert [int(v) for v in out] == [C.sizeof(P), P.width.offset, P.height.offset, P.iterations.offset, P.sigma_color.offset, P.sigma_normal.offset, P.sigma_depth.offset,
                                     P.demodulate.offset, C.sizeof(I), I.sigma_color.offset, I.demodulated.offset, I.guide_spp.offset, I.denoise_ms.offset, I.guides_ms.offset]
    assert C.sizeof(P) == 32 and P._fields_[0][0] == "struct_bytes"


def test_host_header_film_requests_compile(H, tmp_path):
    """a small program against jetpbrt.h: RequestDenoise (defaults and options), RequestGuides, Albedo / Normal / Depth"""
    src = r'''
    #include "jetpbrt.h"
    using namespace jetpbrt;
    int main()
    {
        FFilm a(8, 6), b(8, 6), c(8, 6);
        a.RequestDenoise();
        FDenoiseOptions o; o.iterations = 3; o.sigmaColor = 0.5f; o.demodulate = false;
        b.RequestDenoise(4, o);
        c.RequestGuides(2);
        if (!a.wantDenoise || !a.wantGuides || a.guideSpp_ != 8 || b.denoise.iterations != 3 || c.wantDenoise || !c.wantGuides) return 1;
        const std::vector<FColor>& al = a.Albedo(); const std::vector<FVector3>& n = a.Normal(); const std::vector<Float>& z = a.Depth();
        return (int)(al.size() + n.size() + z.size());     // nothing rendered: the guides are empty
    }'''
    host = os.path.join(H.REPO, "jet-pbrt_amd", "host")
    open(tmp_path / "t.cc", "w").write(src)
    subprocess.run(["g++", "-std=c++17", "-I", host, "-I", os.path.join(H.REPO, "include"), str(tmp_path / "t.cc"), "-o", str(tmp_path / "t"),
                    "-L", host, "-ljetpbrt_host", "-Wl,-rpath," + host, "-ldl", "-lpthread"], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_cli_denoise_flags(H):
    r = subprocess.run([jp.CLI_PATH], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0
    for flag in ("--denoise", "--guide-spp", "--aov"):
        assert flag in r.stderr, flag
    for bad in ("0", "1025", "-3"):
        r = subprocess.run([jp.CLI_PATH, "0", "4", "16", "16", "--guide-spp", bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 5 and "--guide-spp" in r.stderr, bad


FILTER_SIZES = [(1, 1), (3, 7), (67, 129), (256, 256), (200, 333)]          # (H, W); 333 x 200: no multiple of any tile
SIGMAS = [(1.0, 0.3, 0.1), (0.25, 0.1, 0.02)]


@pytest.mark.parametrize("size", FILTER_SIZES[:3] + [(96, 128)])
def test_numpy_restatement_raises_no_fp_exception(size):
    """the reference the device is held to must itself be free of NaN / inf / division by zero on the GPU tests' inputs (underflow of a tiny weight
    is benign), and it must do something: on flat guides it averages, across a guide edge it does not"""
    Hh, W = size
    film, albedo, normal, depth = R.filter_inputs(Hh, W, 7)
    for it in (1, 6):
        for demod in (True, False):
            for sg in SIGMAS:
                with np.errstate(over="raise", invalid="raise", divide="raise"):
                    out = R.atrous_ref(film, albedo, normal, depth, it, *sg, demodulate=demod)
                assert out.dtype == f32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1


def test_numpy_restatement_smooths_flat_regions_and_keeps_edges():
    rng = np.random.default_rng(0)
    Hh, W = 64, 64
    base = np.full((Hh, W, 3), 0.5, f32)
    film = (base * (0.5 + rng.random((Hh, W, 3), dtype=f32))).astype(f32)
    one = np.ones((Hh, W, 3), f32); n = np.zeros((Hh, W, 3), f32); n[..., 2] = 1; z = np.full((Hh, W), 5.0, f32)
    out = R.atrous_ref(film, one, n, z, 5, 4.0, 0.3, 0.1)
    assert ((out - base) ** 2).mean() < 0.1 * ((film - base) ** 2).mean()
    # a depth edge between a dark and a bright half survives
    film2 = film.copy(); film2[:, W // 2:] *= f32(0.1); z2 = z.copy(); z2[:, W // 2:] = 50
    out2 = R.atrous_ref(film2, one, n, z2, 5, 4.0, 0.3, 0.1)
    assert out2[:, :W // 2].mean() > 5 * out2[:, W // 2:].mean()
    # 1 x 1: the centre tap alone, out = Clamp01((film / a) * a)
    f1 = np.array([[[0.25, 0.5, 2.0]]], f32)
    assert np.array_equal(R.atrous_ref(f1, np.ones((1, 1, 3), f32), np.zeros((1, 1, 3), f32), np.zeros((1, 1), f32), 6), np.array([[[0.25, 0.5, 1.0]]], f32))


def test_counter_sampler_restatement_matches_the_header(H, tmp_path):
    """the uint32 restatement of include/jp_counter_rng.h the guide tests build their camera rays from, against the header compiled as C"""
    src = r'''
    #include "jp_counter_rng.h"
    #include <stdio.h>
    int main(){ for (unsigned s = 0; s < 3; s++) for (unsigned y = 0; y < 5; y++) for (unsigned x = 0; x < 7; x++) { unsigned k = jp_rng_key(1234u, x, y, s);
        printf("%u %.9g %.9g\n", k, jp_rng_float(k, 0), jp_rng_float(k, 1)); } return 0; }'''
    open(tmp_path / "r.c", "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), str(tmp_path / "r.c"), "-o", str(tmp_path / "r")], check=True)
    rows = np.array([l.split() for l in subprocess.run([str(tmp_path / "r")], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().split("\n")])
    i = 0
    with np.errstate(over="ignore"):
        for s in range(3):
            yy, xx = np.mgrid[0:5, 0:7]
            k = R.rng_key(1234, xx.ravel(), yy.ravel(), s)
            want = rows[i:i + 35]; i += 35
            assert np.array_equal(k, want[:, 0].astype(np.uint64).astype(np.uint32))
            assert np.array_equal(R.rng_float(k, 0), want[:, 1].astype(f32)) and np.array_equal(R.rng_float(k, 1), want[:, 2].astype(f32))
