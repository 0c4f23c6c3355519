"""The estimator's restatement (tests/mis_ref.py) checked against what can be known without a GPU: both single-point estimators against Lambert's
polygon formula, the weight function's fixed points, the variance ratios the GPU tests' scenes are built for, and the command line switch."""
import subprocess

import numpy as np
import pytest

import jet_pbrt_amd as jp
import mis_ref as M

N = 10 ** 6


def test_weight_fixed_points():
    assert M.weight(2.0, 0.0) == 1.0 and M.weight(1.0, 1.0) == 0.5 and M.weight(1.0, np.inf) == 0.0
    a, b = 3.0, 0.25
    assert np.isclose(M.weight(a, b) + M.weight(b, a), 1.0, rtol=1e-15)
    assert np.isclose(M.weight(a, b), a * a / (a * a + b * b), rtol=1e-15)
    assert np.isfinite(M.weight(1e30, 1e30)) and M.weight(1e30, 1e30) == 0.5       # no inf / inf


@pytest.mark.parametrize("x,z", [(0.0, 0.0), (0.7, 0.5)])
def test_both_estimators_agree_with_the_polygon_formula(x, z):
    r = M.lamp_prediction(x, z)
    cf = M.lamp_closed_form(x, z)
    for k in ("nee", "mis"):
        mean, var = r[k]
        se = np.sqrt(var / N)
        print("matte point (%.1f, %.1f) below the lamp, %s: mean %.6f, closed form %.6f, z = %+.2f" % (x, z, k, mean, cf, (mean - cf) / se))
        assert abs(mean - cf) <= 5.0 * se, (k, mean, cf, se)


def test_polygon_formula_limits():
    # an infinite plane of radiance 1 gives irradiance pi; a small far square A cos cos / d^2
    big = np.array([[1e6, 1.0, -1e6], [-1e6, 1.0, -1e6], [-1e6, 1.0, 1e6], [1e6, 1.0, 1e6]])
    assert np.isclose(M.polygon_irradiance(big, np.zeros((1, 3)), np.array([0.0, 1.0, 0.0]))[0], np.pi, rtol=1e-5)
    sm = np.array([[0.01, 10.0, -0.01], [-0.01, 10.0, -0.01], [-0.01, 10.0, 0.01], [0.01, 10.0, 0.01]])
    assert np.isclose(M.polygon_irradiance(sm, np.zeros((1, 3)), np.array([0.0, 1.0, 0.0]))[0], 4e-4 / 100.0, rtol=1e-5)


def test_metal_estimators_agree_with_each_other():
    r = M.metal_prediction()
    z = (r["mis"][0] - r["nee"][0]) / np.sqrt((r["mis"][1] + r["nee"][1]) / N)
    print("metal point: nee %.6f, mis %.6f, z = %+.2f" % (r["nee"][0], r["mis"][0], z))
    assert abs(z) <= 5.0


def test_predicted_variance_ratios():
    lamp = M.lamp_prediction(); metal = M.metal_prediction()
    rl, rm = lamp["mis"][1] / lamp["nee"][1], metal["mis"][1] / metal["nee"][1]
    print("predicted per-sample variance MIS / NEE: lamp %.3e, metal %.3e" % (rl, rm))
    assert rl <= 0.25 and rm <= 0.1


def test_command_line_switch_parses():
    # without a scene id the command line parses its switches and leaves (main.cc:122-125): no GPU needed
    for mode in ("nee", "mis"):
        assert subprocess.run([jp.CLI_PATH, "--estimator", mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 0
    r = subprocess.run([jp.CLI_PATH, "--estimator", "bogus"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 5 and "--estimator must be nee or mis" in r.stderr


def test_bindings_declare_the_estimator():
    L = jp.hip_lib()
    assert L.jp_set_estimator(None, None) == -1 and b"jp_set_estimator" in L.jp_last_error()      # null context: refused before any device call
    assert jp.ESTIMATOR_MODES["mis"] == jp.JP_ESTIMATOR_MIS == 1 and jp.ESTIMATOR_MODES[None] == jp.JP_ESTIMATOR_NEE == 0
