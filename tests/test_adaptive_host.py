"""Adaptive sampling, the part that needs no GPU: jp_adaptive_samples (pure host code, the functions the device runs) against its numpy restatement bit for
bit -- film, counts and variance -- on synthetic samples whose surviving set after the first test is chosen pixel by pixel, and jp_check_adaptive."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import adaptive_ref as A

f32 = np.float32
H, W = A.H, A.W
MIN, STEP, MAX = 4, 4, 14                                                    # MAX - MIN is no multiple of STEP: the last pass is short (counts 4, 8, 12, 14)
THR = 0.05


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[2]), _bits(want[2]))


def _run(s, dilate, film=None, min_spp=MIN, step=STEP, thr=THR, floor=0.0):
    a = jp.adaptive(thr, min_spp, step, s.shape[0], floor, dilate)
    trace = []
    want = A.adaptive_ref(s, H, W, min_spp, step, thr, floor, dilate, film.sample_clamp if film else 0.0, film.hdr if film else 0, trace)
    got = jp.adaptive_samples(film, a, s, H, W)
    _same(got, want)
    return got, trace


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("k", A.SURVIVORS)
def test_samples_equal_the_restatement(k, dilate):
    """the surviving set after the first test has exactly k pixels under dilate = 0; dilate = 1 keeps their 3 x 3 neighbourhoods too (a set of one pixel cannot
    survive alone under it), whose size the restatement gives: the clipped dilation of the same set"""
    noisy = A.survivor_pixels(k)
    (film, counts, var), trace = _run(A.synthetic_samples(noisy, MAX), dilate)
    if k == 0:
        assert trace == [0] and (counts == MIN).all()
    elif dilate == 0:
        assert trace == [k] * 3                                              # tests after 4, 8 and 12 samples: an alternating pixel never passes
        assert (counts.reshape(-1)[noisy] == MAX).all() and (counts == MIN).sum() == H * W - k
    else:
        mask = np.zeros(H * W, bool); mask[noisy] = True
        grown = A.fails_nearby(mask.reshape(H, W))
        assert trace == [int(grown.sum())] * 3 and np.array_equal(counts == MAX, grown)
    assert (var.reshape(-1)[np.setdiff1d(np.arange(H * W), noisy)] == 0).all()


@pytest.mark.parametrize("pixel", [0, W - 1, (H - 1) * W, H * W - 1, 5, 7 * W, 8 * W - 1, (H - 1) * W + 11])
def test_one_survivor_at_a_corner_or_an_edge(pixel):
    (_, counts, _), trace = _run(A.synthetic_samples([pixel], MAX), 0)
    assert trace == [1, 1, 1] and counts.reshape(-1)[pixel] == MAX and (counts == MAX).sum() == 1
    (_, counts, _), trace = _run(A.synthetic_samples([pixel], MAX), 1)       # the clipped neighbourhood: 4 pixels at a corner, 6 on an edge
    y, x = divmod(pixel, W)
    want = (min(y + 1, H - 1) - max(y - 1, 0) + 1) * (min(x + 1, W - 1) - max(x - 1, 0) + 1)
    assert trace == [want] * 3 and (counts == MAX).sum() == want


def test_dilation_can_leave_out_exactly_one_pixel():
    """everything is noisy but the 2 x 2 block in the corner: under dilate = 1 only the corner pixel itself has no noisy neighbour"""
    quiet = [0, 1, W, W + 1]
    noisy = np.setdiff1d(np.arange(H * W), quiet)
    (_, counts, _), trace = _run(A.synthetic_samples(noisy, MAX), 1)
    assert trace == [H * W - 1] * 3 and counts[0, 0] == MIN and (counts == MAX).sum() == H * W - 1


@pytest.mark.parametrize("hdr", [0, 1])
@pytest.mark.parametrize("clamp", [0.0, 1.5])
@pytest.mark.parametrize("dilate", [0, 1])
def test_film_state_and_hostile_samples(dilate, clamp, hdr):
    s = A.synthetic_samples(A.survivor_pixels(257), MAX, hostile=True)
    big = A.survivor_pixels(257)[3]
    s[::2, big] = f32(3e30); s[1::2, big] = 0                                # m2 overflows: the test's left side is infinite, which counts as a pass
    (film, counts, var), _ = _run(s, dilate, jp.film(hdr, clamp))
    assert (film >= 0).all() and not np.isnan(film).any()
    if clamp == 0:
        assert not np.isfinite(var.reshape(-1)[big])
        if dilate == 0:
            assert counts.reshape(-1)[big] == MIN
    else:
        assert np.isfinite(var).all()
    quiet0 = np.setdiff1d(np.arange(H * W), A.survivor_pixels(257))[0]       # the constant pixel (3, 0.5, 2)
    want = np.array([3.0, 0.5, 2.0], f32)
    if clamp > 0:
        want = (want * (f32(clamp) / f32(3.0))).astype(f32)
    if not hdr:
        want = np.minimum(want, f32(1))
    assert np.array_equal(film.reshape(-1, 3)[quiet0], want)


@pytest.mark.parametrize("dilate", [0, 1])
def test_counts_are_monotone_steps(dilate):
    """random samples whose noise differs from pixel to pixel: pixels stop at different tests, and a count is min + k * step or max, nothing else"""
    rng = np.random.default_rng(11)
    sigma = (f32(10.0) ** rng.uniform(-2.5, 0, (1, H * W, 1))).astype(f32)
    s = np.abs(f32(0.5) + sigma * rng.standard_normal((37, H * W, 3)).astype(f32)).astype(f32)
    (_, counts, var), trace = _run(s, dilate, min_spp=5, step=6, thr=0.03)
    allowed = sorted(set(range(5, 37, 6)) | {37})
    assert set(np.unique(counts)) <= set(allowed) and len(np.unique(counts)) >= 4
    assert trace == sorted(trace, reverse=True) and trace[0] < H * W
    stopped = counts < 37
    t2 = np.square(f32(0.03) * np.maximum(f32(0.4), f32(1e-3)))              # every mean is above 0.4: a pixel that stopped did so below this bound
    if dilate == 0:
        assert (var[stopped] <= 4 * t2).all()


def test_threshold_zero_is_the_uniform_render():
    s = A.synthetic_samples(A.survivor_pixels(255), MAX)
    (film, counts, _), _ = _run(s, 0, thr=0.0)
    assert (counts.reshape(-1)[A.survivor_pixels(255)] == MAX).all()         # (a constant pixel has variance 0 <= 0 and still stops: nothing is left to average)
    s2 = np.abs(np.random.default_rng(2).standard_normal((MAX, H * W, 3))).astype(f32)
    (_, counts, _), _ = _run(s2, 1, thr=0.0)
    assert (counts == MAX).all()


def test_min_equals_max_runs_one_pass():
    s = A.synthetic_samples(A.survivor_pixels(256), 6)
    (_, counts, _), trace = _run(s, 1, min_spp=6, step=3)
    assert trace == [] and (counts == 6).all()


def test_refusals_carry_a_message():
    ok = jp.adaptive(0.05, 8, 8, 32, 0.0, 1)
    jp.check_adaptive(ok)
    jp.check_adaptive(jp.adaptive(0.0, 2, 1, 0, 0.0, 0))                     # max_spp 0: the render's spp
    bad = [(dict(min_spp=1), "min_spp"), (dict(min_spp=0), "min_spp"), (dict(step_spp=0), "step_spp"), (dict(max_spp=7), "max_spp"), (dict(max_spp=-1), "max_spp"),
           (dict(threshold=-0.1), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"),
           (dict(floor=-1.0), "floor"), (dict(floor=float("nan")), "floor"), (dict(dilate=2), "dilate"), (dict(dilate=-1), "dilate"), (dict(struct_bytes=4), "struct_bytes")]
    for change, word in bad:
        a = jp.adaptive(0.05, 8, 8, 32, 0.0, 1)
        for k, v in change.items():
            setattr(a, k, v)
        with pytest.raises(jp.JetPbrtError) as e:
            jp.check_adaptive(a)
        assert "jp_render_adaptive" in str(e.value) and word in str(e.value)
    with pytest.raises(jp.JetPbrtError) as e:
        jp.check_adaptive(None)
    assert "JpAdaptive" in str(e.value)


def test_samples_arguments_are_checked():
    L = jp.hip_lib()
    s = A.synthetic_samples([], MAX)
    out = np.zeros((H, W), f32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    a = jp.adaptive(THR, MIN, STEP, MAX)
    assert L.jp_adaptive_samples(None, C.byref(a), W, H, p(s), None, None, p(out)) == 0
    assert L.jp_adaptive_samples(None, C.byref(a), W, H, p(s), None, None, None) == -1 and b"jp_adaptive_samples" in L.jp_last_error()
    assert L.jp_adaptive_samples(None, C.byref(a), W, H, None, None, None, p(out)) == -1
    assert L.jp_adaptive_samples(None, C.byref(a), 0, H, p(s), None, None, p(out)) == -1
    assert L.jp_adaptive_samples(None, None, W, H, p(s), None, None, p(out)) == -1
    a0 = jp.adaptive(THR, MIN, STEP, 0)
    assert L.jp_adaptive_samples(None, C.byref(a0), W, H, p(s), None, None, p(out)) == -1 and b"max_spp" in L.jp_last_error()
    bad = jp.film(0, -1.0)
    assert L.jp_adaptive_samples(C.byref(bad), C.byref(a), W, H, p(s), None, None, p(out)) == -1
