"""Variance, the part that needs no GPU: jp_variance_samples (pure host code, the function the device runs) against its numpy restatement bit for bit, its
argument checks, and the restatement of the variance-guided filter on hostile variance planes (no floating-point exception)."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import variance_ref as V

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _samples(spp, n, seed):
    """random radiances over several decades with the edge pixels the definition names: 0 a constant pixel, 1 one sample of 1e6, 2 a NaN channel, 3 an
    infinite channel, 4 all zero, 5 a constant pixel that is not representable exactly"""
    rng = np.random.default_rng(seed)
    s = (rng.random((spp, n, 3), dtype=f32) * (f32(10.0) ** rng.integers(-3, 3, (1, n, 1)).astype(f32))).astype(f32)
    s[:, 0] = f32(0.25)
    s[:, 1] = f32(0.5); s[spp // 2, 1] = f32(1e6)
    s[spp - 1, 2, 1] = np.nan
    s[0, 3, 2] = np.inf
    s[:, 4] = 0
    s[:, 5] = np.array([0.1, 0.7, 0.3], f32)
    return s


@pytest.mark.parametrize("clamp", [0.0, 2.5])
@pytest.mark.parametrize("spp", [2, 3, 16, 257])
def test_variance_samples_equal_the_restatement(spp, clamp):
    s = _samples(spp, 301, spp)
    film = jp.film(0, clamp) if clamp > 0 else None
    var, mean = jp.variance_samples(film, s, want_mean=True)
    want_var, want_mean = V.moments_ref(s, clamp)
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert np.array_equal(_bits(var), _bits(want_var))
    assert var[0] == 0 and var[4] == 0 and var[5] == 0                       # a constant pixel: exactly 0
    assert np.isfinite(var).all() and (var >= 0).all() and (var[6:] > 0).all()
    if clamp == 0:
        assert var[1] > 1e6                                                  # one sample of 1e6 among 0.5s: (1e6)^2 / spp^2 at the least
    else:
        assert var[1] < clamp * clamp                                        # ... which the sample clamp takes down to 2.5


def test_a_film_without_a_clamp_is_no_film():
    s = _samples(7, 64, 1)
    assert np.array_equal(_bits(jp.variance_samples(jp.film(1, 0.0), s)), _bits(jp.variance_samples(None, s)))


def test_bessel_and_the_division_by_spp():
    """two samples a, b: the variance of their mean is ((a - b)^2 / 2) / 2"""
    s = np.zeros((2, 1, 3), f32); s[0, 0] = 1; s[1, 0] = 3
    y0, y1 = V._lum(s[0])[0], V._lum(s[1])[0]
    var = jp.variance_samples(None, s)[0]
    assert abs(var - (y0 - y1) ** 2 / 4) < 1e-6 * var


def test_arguments_are_checked():
    L = jp.hip_lib()
    s = _samples(4, 8, 0)
    out = np.zeros(8, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.jp_variance_samples(None, 1, 8, p(s), p(out), None) == -1
    assert b"jp_variance_samples" in L.jp_last_error() and b"spp" in L.jp_last_error()
    assert L.jp_variance_samples(None, 0, 8, p(s), p(out), None) == -1
    assert L.jp_variance_samples(None, 4, 8, None, p(out), None) == -1
    assert L.jp_variance_samples(None, 4, 8, p(s), None, None) == -1
    assert L.jp_variance_samples(None, 4, -1, p(s), p(out), None) == -1
    bad = jp.film(0, -1.0)
    assert L.jp_variance_samples(C.byref(bad), 4, 8, p(s), p(out), None) == -1
    assert L.jp_variance_samples(None, 4, 0, None, None, None) == 0
    assert L.jp_variance_samples(None, 4, 8, p(s), p(out), None) == 0 and np.array_equal(_bits(out), _bits(V.moments_ref(s)[0]))
    mean = np.zeros(8, f32)
    assert L.jp_variance_samples(None, 4, 8, p(s), None, p(mean)) == 0 and np.array_equal(_bits(mean), _bits(V.moments_ref(s)[1]))


@pytest.mark.parametrize("size", [(1, 1), (3, 7), (24, 40)])
def test_filter_restatement_raises_no_floating_point_exception(size):
    h, w = size
    film, albedo, normal, depth = V.filter_inputs(h, w, 7)
    var = V.variance_inputs(h, w, 7)
    if var.size >= 6:                                                        # (a 1 x 1 plane holds one of them)
        assert np.isnan(var).any() and (var[~np.isnan(var)] < 0).any() and (var == 0).any() and (var == f32(1e6)).any()
    for it in (1, 3, 6):
        for demod in (True, False):
            for hdr in (False, True):
                with np.errstate(over="raise", invalid="raise", divide="raise"):
                    out, vout = V.atrous_v_ref(film, albedo, normal, depth, var, it, 2.0, 0.1, 0.03, demodulate=demod, hdr=hdr)
                assert np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all() and (out >= 0).all()
                assert hdr or (out <= 1).all()


def test_a_zero_variance_plane_stops_at_colour_edges_and_a_huge_one_does_not():
    """kc = 1 / (sc2 * g + 1e-8): no variance -> only equal colours mix (the film comes back where neighbours differ); a huge variance -> the colour edge-stop is off
    and the result is the plain weighted mean under the normal and depth stops"""
    h, w = 16, 16
    film, albedo, normal, depth = V.filter_inputs(h, w, 3)
    normal[:] = np.array([0, 0, 1], f32); depth[:] = 10
    sharp, v0 = V.atrous_v_ref(film, albedo, normal, depth, np.zeros((h, w), f32), 3, demodulate=False)
    assert np.abs(sharp - film).max() < 1e-4 and (v0 == 0).all()
    flat, _ = V.atrous_v_ref(film, albedo, normal, depth, np.full((h, w), 1e6, f32), 3, demodulate=False)
    assert flat.std() < 0.5 * film.std()
