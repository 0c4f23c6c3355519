"""The film, host side (no GPU): the exported symbols and the ABI version, the ctypes layout of the new structs against a compiled C probe, the validation
of jp_check_film / jp_check_tonemap, and the pure-host functions -- the very text the device runs -- against the numpy restatement bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
import film_ref as R

f32 = np.float32
INVALID_ARGUMENT = -1
CURVES = [jp.JP_CURVE_CLAMP, jp.JP_CURVE_REINHARD, jp.JP_CURVE_ACES, jp.JP_CURVE_HABLE]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _thresholds():
    thr = np.zeros(255, f32)
    assert jp.hip_lib().jp_gamma_thresholds(thr.ctypes.data_as(C.c_void_p)) == 0
    return thr


def test_film_symbols_exported_and_abi_unchanged():
    lib = jp.hip_lib()
    for name in ("jp_set_film", "jp_check_film", "jp_get_film_info", "jp_film_samples", "jp_film_histogram", "jp_film_histogram_device", "jp_set_tonemap",
                 "jp_check_tonemap", "jp_exposure_from_histogram", "jp_tonemap", "jp_tonemap_device", "jp_tonemap_host", "jp_get_tonemap_info"):
        assert hasattr(lib, name), name
    assert lib.jp_abi_version() == 7 and jp.JP_ABI_VERSION == 7
    for name in ("set_film", "film_info", "set_tonemap", "tonemap_info", "film_histogram", "tonemap"):
        assert callable(getattr(jp.Context, name)), name


def test_film_struct_layouts_match_the_header(H, tmp_path):
    structs = {"JpFilm": jp.JpFilm, "JpFilmInfo": jp.JpFilmInfo, "JpToneMap": jp.JpToneMap, "JpToneMapInfo": jp.JpToneMapInfo}
    probes, want = [], []
    for name, S in structs.items():
        probes.append("sizeof(%s)" % name); want.append(C.sizeof(S))
        for field, _ in S._fields_:
            probes.append("offsetof(%s, %s)" % (name, field)); want.append(getattr(S, field).offset)
    src = '#include "jetpbrt_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){ size_t v[] = { %s }; for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu\\n", v[i]); return JP_FILM_BINS != 256; }' % ", ".join(probes)
    open(tmp_path / "t.c", "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(H.REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(v) for v in out] == want
    assert C.sizeof(jp.JpFilm) == 12 and C.sizeof(jp.JpToneMap) == 32 and jp.JP_FILM_BINS == 256
    for S in structs.values():
        assert S._fields_[0][0] == "struct_bytes"


def test_shared_headers_compile_as_c(H, tmp_path):
    """include/jp_film.h and include/jp_tonemap.h are plain C99 as well: a C program gets the library's answers from them"""
    src = r'''
    #include "jp_tonemap.h"
    #include <stdio.h>
    int main(){ float r = 8.f, g = 2.f, b = 1.f; jp_film_clamp_sample(2.f, &r, &g, &b);
        printf("%.9g %.9g %.9g %d %d %.9g\n", r, g, b, jp_film_bin(1.f, 1.f, 1.f), jp_film_bin(0.f, -1.f, 0.f), jp_tm_value(JP_CURVE_ACES, 16.f, 1.f, 0.5f)); return 0; }'''
    open(tmp_path / "t.c", "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(H.REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t"), "-lm"], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    want = R.sample_clamp(2.0, [[8.0, 2.0, 1.0]])[0]
    assert _same(np.array(out[:3], f32), want)
    assert int(out[3]) == int(np.argmax(R.histogram([[1.0, 1.0, 1.0]]))) and int(out[4]) == R.BINS
    assert _same(np.array(out[5:], f32), R.curve_values(jp.tonemap("aces"), 1.0, [0.5]))


def _refused(call, needle):
    L = jp.hip_lib()
    assert call() == INVALID_ARGUMENT
    assert needle in L.jp_last_error().decode(), L.jp_last_error().decode()


def test_check_film_refuses_each_bad_field():
    L = jp.hip_lib()
    assert L.jp_check_film(None) == 0
    for ok in (jp.film(0, 0.0), jp.film(1, 0.0), jp.film(1, 2.5), jp.film(0, 1e-30)):
        assert L.jp_check_film(C.byref(ok)) == 0
    _refused(lambda: L.jp_check_film(C.byref(jp.JpFilm(4, 1, 0.0))), "struct_bytes")
    for hdr in (-1, 2):
        _refused(lambda: L.jp_check_film(C.byref(jp.film(hdr, 0.0))), "hdr")
    for c in (-1.0, float("nan"), float("inf"), -float("inf")):
        _refused(lambda: L.jp_check_film(C.byref(jp.film(1, c))), "sample_clamp")
        with pytest.raises(jp.JetPbrtError, match="sample_clamp"):
            jp.check_film(jp.film(1, c))
        _refused(lambda: L.jp_film_samples(C.byref(jp.film(1, c)), 0, None, None), "sample_clamp")


def test_check_tonemap_refuses_each_bad_field():
    L = jp.hip_lib()
    assert L.jp_check_tonemap(None) == 0
    for ok in (jp.tonemap(), jp.tonemap("hable", "auto", -3.0, 0.5, 11.2, 0.25, 1.0), jp.tonemap("reinhard", pct_high=0.06)):
        assert L.jp_check_tonemap(C.byref(ok)) == 0
    nan, inf = float("nan"), float("inf")
    bad = [(jp.JpToneMap(28, 0, 0, 0, 0, 0, 0, 0), "struct_bytes"), (jp.tonemap(-1), "curve"), (jp.tonemap(4), "curve"), (jp.tonemap(0, 2), "exposure_mode"),
           (jp.tonemap(0, -1), "exposure_mode")]
    bad += [(jp.tonemap(ev=v), "ev") for v in (nan, inf, -inf)]
    bad += [(jp.tonemap(key=v), "key") for v in (-0.18, nan, inf)]
    bad += [(jp.tonemap(white=v), "white") for v in (-4.0, nan, inf)]
    bad += [(jp.tonemap(pct_low=v), "percentiles") for v in (-0.1, 0.95, 0.99, nan, inf)]          # 0.95: not below the default pct_high
    bad += [(jp.tonemap(pct_high=v), "percentiles") for v in (1.5, 0.05, 0.01, nan, -0.5)]          # 0.05: not above the default pct_low
    s = C.c_float(0)
    hist = np.zeros(R.BINS + 1, np.uint32)
    x = np.zeros(3, f32); y = np.zeros(3, f32)
    for t, needle in bad:
        _refused(lambda: L.jp_check_tonemap(C.byref(t)), needle)
        _refused(lambda: L.jp_exposure_from_histogram(C.byref(t), hist.ctypes.data_as(C.c_void_p), C.byref(s)), needle)
        _refused(lambda: L.jp_tonemap_host(C.byref(t), C.c_float(1.0), 3, x.ctypes.data_as(C.c_void_p), None, y.ctypes.data_as(C.c_void_p)), needle)
        with pytest.raises(jp.JetPbrtError, match=needle):
            jp.check_tonemap(t)
    _refused(lambda: L.jp_exposure_from_histogram(C.byref(jp.tonemap(exposure="auto")), None, C.byref(s)), "histogram")


def test_film_samples_is_the_restatement():
    v = R.adversarial_values()
    rng = np.random.default_rng(3)
    rgb = np.stack([v, rng.permutation(v), rng.permutation(v)], axis=1)
    for c in (2.0, 0.18, 1e-3, 1e9, 3.0e38):
        got = jp.film_samples(jp.film(1, c), rgb)
        want = R.sample_clamp(c, rgb)
        assert _same(got, want), c
        fin = np.isfinite(rgb).all(axis=1)
        assert (got[~fin] == 0).all() and (got[fin].max(axis=1) <= f32(c) * (1 + 2.0 ** -23)).all()
    # off: a copy, NaN and all
    assert _same(jp.film_samples(None, rgb), rgb) and _same(jp.film_samples(jp.film(1, 0.0), rgb), rgb)
    # the definition on a value one can check by hand: m = 8 > 2 -> k = 0.25
    assert _same(jp.film_samples(jp.film(0, 2.0), [[8.0, 2.0, 1.0], [1.0, 2.0, 0.5], [np.inf, 0.0, 0.0]]), [[2.0, 0.5, 0.25], [1.0, 2.0, 0.5], [0.0, 0.0, 0.0]])


@pytest.mark.parametrize("curve", CURVES)
def test_tonemap_host_is_the_restatement(curve):
    v = R.adversarial_values()
    thr = _thresholds()
    for ev in (-2.0, 0.0, 3.0):
        for white in (0.0, 1.5):
            t = jp.tonemap(curve, "manual", ev, white=white)
            scale = jp.exposure_from_histogram(t, None)
            assert scale == 2.0 ** ev
            b, y = jp.tonemap_host(t, scale, v)
            want = R.curve_values(t, scale, v)
            assert _same(y, want), (curve, ev, white)
            assert np.array_equal(b, R.gamma_bytes(thr, want))
            assert y.min() >= 0 and y.max() <= 1 and np.isfinite(y).all()
    # bytes alone, floats alone
    t = jp.tonemap(curve)
    b2, none = jp.tonemap_host(t, 1.0, v, want_floats=False)
    none2, y2 = jp.tonemap_host(t, 1.0, v, want_bytes=False)
    assert none is None and none2 is None and np.array_equal(b2, R.gamma_bytes(thr, y2))


def test_clamp_manual_ev0_bytes_are_the_threshold_table():
    """CLAMP, MANUAL, ev 0: the bytes jp_render_rgb8 gives -- the number of gamma thresholds <= Clamp01(x) -- for the whole vector"""
    v = R.adversarial_values()
    thr = _thresholds()
    b, y = jp.tonemap_host(jp.tonemap(), 1.0, v)
    with np.errstate(invalid="ignore"):
        clamped = np.where(v > 0, np.minimum(v, f32(1)), f32(0)).astype(f32)       # Clamp01 with NaN and -0 at 0
    assert _same(y, clamped)
    assert np.array_equal(b, (thr[None, :] <= clamped[:, None]).sum(axis=1).astype(np.uint8))
    assert b.min() == 0 and b.max() == 255


def _hists():
    rng = np.random.default_rng(11)
    out = []
    h = np.zeros(R.BINS + 1, np.uint32); h[100:140] = rng.integers(1, 5000, 40); h[R.BINS] = 77; out.append(h)
    h = rng.integers(0, 3, R.BINS + 1).astype(np.uint32); out.append(h)                                # sparse, small counts: the ends fall inside bins
    h = np.zeros(R.BINS + 1, np.uint32); h[0] = 10; h[255] = 10; h[128] = 1; out.append(h)             # both ends of the range
    h = np.zeros(R.BINS + 1, np.uint32); h[120:136] = 1 << 27; out.append(h)                            # 2^31 pixels in all
    return out


def test_exposure_from_histogram_matches_float64_restatement():
    tms = [jp.tonemap(exposure="auto"), jp.tonemap("aces", "auto", 1.5), jp.tonemap("hable", "auto", -2.0, key=0.36, pct_low=0.25, pct_high=0.5),
           jp.tonemap("reinhard", "auto", 0.0, pct_low=0.001, pct_high=1.0), jp.tonemap(exposure="manual", ev=2.5)]
    for h in _hists():
        for t in tms:
            got = jp.exposure_from_histogram(t, h)
            want = R.exposure(t, h)
            # a few hundred double operations of at most 1 ulp each stay below 1e-13, libm's log2 / exp2 add a few ulp: 1e-12 relative.  (Both sides round
            # their double to fp32 last, so this asks for the same fp32 value.)
            assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (got, want)
            assert np.isfinite(got) and got > 0


def test_exposure_double_path_within_1e12(H, tmp_path):
    """the same comparison on the header compiled as C: its value against the restatement within 1e-12 relative, and the library gives that very value"""
    src = r'''
    #include "jp_tonemap.h"
    #include <stdio.h>
    int main(){ uint32_t h[JP_FILM_BINS + 1]; for (int k = 0; k <= JP_FILM_BINS; k++) h[k] = (uint32_t)((k * 2654435761u) >> 20) % 997u;
        JpToneMap in = { sizeof(JpToneMap), JP_CURVE_ACES, JP_EXPOSURE_AUTO, 0.75f, 0.f, 0.f, 0.1f, 0.9f }, tm;
        if (jp_tonemap_resolve(&in, &tm)) return 1;
        printf("%.9g\n", jp_tonemap_exposure(&tm, h)); return 0; }'''
    open(tmp_path / "t.c", "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(H.REPO, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t"), "-lm"], check=True)
    got = float(f32(subprocess.run([str(tmp_path / "t")], check=True, stdout=subprocess.PIPE, text=True).stdout))     # nine digits name the fp32 value
    k = np.arange(R.BINS + 1, dtype=np.uint64)
    h = ((((k * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(20)) % np.uint64(997)).astype(np.uint32)
    t = jp.tonemap("aces", "auto", 0.75, pct_low=0.1, pct_high=0.9)
    want = R.exposure(t, h)
    assert abs(got - float(want)) <= 1e-12 * abs(float(want))
    assert jp.exposure_from_histogram(t, h) == f32(got)                    # the library runs the header's text


def test_degenerate_histograms():
    t = jp.tonemap("aces", "auto", 0.0)
    zero = np.zeros(R.BINS + 1, np.uint32)
    assert jp.exposure_from_histogram(t, zero) == 1.0 and R.exposure(t, zero) == 1.0
    excl = zero.copy(); excl[R.BINS] = 123456
    assert jp.exposure_from_histogram(t, excl) == 1.0 and R.exposure(t, excl) == 1.0
    # ev still has no say where nothing was measured
    assert jp.exposure_from_histogram(jp.tonemap("aces", "auto", 3.0), excl) == 1.0
    # a single bin: the trimmed count is (pct_high - pct_low) * N of that bin, so Lavg is its centre exactly and the scale key / centre.  (The scale is 1
    # only where nothing is counted -- N == 0 or an empty trimmed span -- which the definition's percentiles cannot produce from a non-empty bin.)
    for k in (0, 127, 128, 131, 255):
        one = zero.copy(); one[k] = 1000
        centre = (1.125 + 0.25 * (k & 3)) * 2.0 ** ((k >> 2) - 32)
        got = jp.exposure_from_histogram(t, one)
        assert got == R.exposure(t, one) and abs(float(got) - 0.18 / centre) <= 2.0 ** -22 * 0.18 / centre
    # bin 128 is [1, 1.25): a key of 1.125 maps it onto itself
    one = zero.copy(); one[128] = 5
    assert jp.exposure_from_histogram(jp.tonemap("aces", "auto", 0.0, key=1.125), one) == 1.0


def test_histogram_restatement_bins():
    """the restatement itself on values one can check by hand: four bins per octave from 2^-32, the ends clamp, zeros / negatives / non-finite are excluded"""
    def bin_of(y):
        h = R.histogram(np.array([[y, y, y]], f32))           # Y = y * (0.2126 + 0.7152 + 0.0722) within an ulp: use values well inside a bin
        return int(np.argmax(h))
    assert bin_of(1.1) == 128 and bin_of(1.3) == 129 and bin_of(1.6) == 130 and bin_of(1.9) == 131 and bin_of(2.2) == 132
    assert bin_of(2.0 ** -32 * 1.1) == 0 and bin_of(2.0 ** -40) == 0 and bin_of(1e-45) == 0 and bin_of(2.0 ** 31 * 1.9) == 255 and bin_of(1e38) == 255
    for y in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        assert bin_of(y) == R.BINS, y
    v = R.adversarial_values().reshape(-1, 3)
    h = R.histogram(v)
    assert int(h.sum()) == len(v) and h[R.BINS] > 0 and h[0] > 0 and h[255] > 0
