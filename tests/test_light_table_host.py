"""The alias table of JP_LIGHTS_POWER_ONE (jp_build_light_table, INTEGRATION.md "Light selection") on the host: no GPU needed.
`check_table` is the definition's checklist; tests/test_gpu_light_pick.py applies it to the table an upload leaves on the device."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp

EPS = 2.0 ** -23      # every fp32 threshold is off by at most 2^-24, and at most n bins of width 1/n add up


def total(w):
    """W: the weights summed in index order, in double (np.cumsum accumulates sequentially; np.sum would sum pairwise)"""
    w = np.asarray(w, np.float64)
    return float(np.cumsum(w)[-1]) if w.size else 0.0


def check_table(w, q, alias, pmf):
    w = np.asarray(w, np.float64); n = w.size
    assert q.dtype == np.float32 and pmf.dtype == np.float32 and alias.dtype == np.int32
    assert q.shape == alias.shape == pmf.shape == (n,)
    W = total(w)
    if n == 0:
        return
    if W == 0.0:
        assert not pmf.any()
        return
    assert np.array_equal(pmf, (w / W).astype(np.float32)), "pmf_i == float32(w_i / W)"
    assert (q >= 0).all() and (q <= 1).all() and (alias >= 0).all() and (alias < n).all()
    qd = q.astype(np.float64)
    implied = (qd + np.bincount(alias, weights=1.0 - qd, minlength=n)) / n
    err = np.abs(implied - w / W)
    print("n = %d: largest |implied - w / W| = %.3e (bound %.3e)" % (n, err.max(), EPS))
    assert err.max() <= EPS
    # no bin can yield a light of weight 0: not through its alias, not by itself
    assert ((q == 1) | (w[alias] > 0)).all()
    assert ((q == 0) | (w > 0)).all()


def _cases():
    rng = np.random.default_rng(20240607)
    one = np.zeros(5); one[3] = 7.25
    logu = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 100000)); logu[rng.random(100000) < 0.1] = 0.0
    return {"random_66": rng.uniform(0.0, 50.0, 66), "one_of_5": one, "equal_8": np.full(8, 3.5), "log_uniform_100000": logu}


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_reproduces_the_pmf(name):
    w = CASES[name]
    q, alias, pmf = jp.build_light_table(w)
    check_table(w, q, alias, pmf)
    if name == "log_uniform_100000":
        assert (w == 0).sum() > 9000                                   # the 10 % of weight 0 are really there
    if name == "one_of_5":
        assert np.array_equal(pmf, np.array([0, 0, 0, 1, 0], np.float32))
        i = np.arange(5); picked = np.where(0.5 < q, i, alias)          # any u1: every bin ends at light 3
        assert (picked == 3).all() and (np.where(0.0 < q, i, alias) == 3).all()
    if name == "equal_8":
        assert (q == 1).all() and np.array_equal(pmf, np.full(8, 0.125, np.float32))


def test_zero_total_and_empty_are_ok():
    L = jp.hip_lib()
    q, alias, pmf = jp.build_light_table(np.zeros(6))
    assert not pmf.any() and not q.any()
    check_table(np.zeros(6), q, alias, pmf)
    assert L.jp_build_light_table(0, None, None, None, None) == jp.JP_OK
    q, alias, pmf = jp.build_light_table(np.zeros(0))
    assert q.size == alias.size == pmf.size == 0


def test_bad_weights_are_refused():
    L = jp.hip_lib()
    for bad in (-1.0, float("nan"), float("inf")):
        w = np.array([1.0, bad, 2.0]); out = np.zeros(3, np.float32); al = np.zeros(3, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.jp_build_light_table(3, p(w), p(out), p(al), p(out.copy())) == -1      # JP_ERR_INVALID_ARGUMENT
    assert L.jp_build_light_table(-1, None, None, None, None) == -1
