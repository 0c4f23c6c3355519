"""Who owns device memory ("Who owns device memory"): every allocation of the library is counted by jp.device_bytes_in_use(), so
"nothing leaks" is an assertion.  Each test has a context of its own -- the session's gpu_ctx would move the baseline -- and every check is the exact
equality of two counter readings.  All frames are 32 x 24 at 4 spp."""
import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes

pytestmark = pytest.mark.gpu
W, HH, SPP = 32, 24, 4


@pytest.fixture(scope="module")
def scene_a():
    be = scenes.build_cornell(scenes.HostBackend("a"), W, HH, lambert_only=False)
    return be, be.flatten()


@pytest.fixture(scope="module")
def scene_b():
    """the textured Cornell box: a checker on the back wall, an image on the floor"""
    img = np.random.default_rng(3).integers(0, 256, (23, 37, 3), dtype=np.uint8)
    be = scenes.build_textured_cornell(scenes.HostBackend("b"), W, HH, back=lambda b: b.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8)), floor=lambda b: b.texture_image(img))
    return be, be.flatten(), be.flatten_textures()


def _params(w=W, h=HH):
    return jp.render_params(w, h, SPP, 5, 1234)


def test_a_closed_context_returns_every_byte(H, scene_a, scene_b, tmp_path):
    b0 = jp.device_bytes_in_use()
    ctx = jp.Context(0)
    try:
        assert jp.device_bytes_in_use() > b0                              # (the counters of the context: the counter counts)
        p = _params()
        # the per-bounce schedule, the 8-bit film, the fused schedule, three stream lanes
        ctx.upload(scene_a[1])
        ctx.render(p); ctx.render_rgb8(p)
        ctx.set_options(fused=1); ctx.render(p)
        assert ctx.build_info().fused_last_render == 1
        ctx.set_options(); ctx.set_options(lanes=3); ctx.render(p)                 # (set_options changes fields of the options in force: back to the defaults first)
        assert ctx.build_info().lanes_last_render == 3
        ctx.set_options()
        # textures: the five texture tables and the side array
        ctx.upload(scene_b[1], scene_b[2]); ctx.render(p)
        assert ctx.texture_info().textured_last_render == 1
        rng = np.random.default_rng(5)
        n = 1000
        o = np.tile(np.array([278, 273, 960], np.float32), (n, 1)); d = rng.normal(size=(n, 3)).astype(np.float32); d[:, 2] = -np.abs(d[:, 2]) - 1
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        t0 = np.full(n, 1e-3, np.float32); t1 = np.full(n, np.inf, np.float32)
        ctx.trace(o, d, t0, t1); ctx.surface(o, d, t0, t1)
        # one light per bounce: the three pick tables
        ctx.set_light_sampling("power")
        ctx.upload(scene_a[1]); ctx.render(p)
        assert ctx.light_info().picked_last_render == 1
        ctx.light_pick(rng.random(n).astype(np.float32), rng.random(n).astype(np.float32))
        ctx.set_light_sampling(None)
        # guides, denoiser, BSDF scratch
        ctx.upload(scene_a[1])
        film = ctx.render(p)
        alb, nrm, dep = ctx.render_guides(p, 4)
        ctx.denoise(film, alb, nrm, dep)
        ctx.bsdf(jp.bsdf_desc(jp.JP_BSDF_LAMBERT), *H.bsdf_inputs(300, 1))
        # the device builds: binary tree (PLOC, then LBVH), 8-wide and 4-wide trees (the latter: more than 1024 primitives)
        hb = scenes.HostBackend("soup"); hb.set_device_build(True)
        H.build_random_scene(hb, W, HH, 21, n_tris=1032, tmpdir=str(tmp_path))
        sp = hb.flatten()
        assert sp.contents.n_primitives > 1024
        for tree in (0, 2):
            ctx.set_options(device_tree=tree)
            ctx.upload(sp)
            bi = ctx.build_info()
            assert bi.built_on_device == 1 and bi.q4_nodes > 0 and bi.traversal_mode == 3
            ctx.render(p)
        ctx.set_options()
        assert jp.device_bytes_in_use() > b0
    finally:
        ctx.close()
    assert jp.device_bytes_in_use() == b0


def test_uploads_and_renders_do_not_accumulate(scene_a, scene_b):
    ctx = jp.Context(0)
    try:
        p = _params()

        def cycle():
            ctx.upload(scene_a[1]); ctx.render(p)
            ctx.upload(scene_b[1], scene_b[2]); ctx.render(p)
            return jp.device_bytes_in_use()
        first = cycle()
        assert cycle() == first
        ctx.render(p)
        assert jp.device_bytes_in_use() == first
        ctx.render(p)
        assert jp.device_bytes_in_use() == first
    finally:
        ctx.close()


def test_a_smaller_frame_reallocates_nothing(scene_a):
    ctx = jp.Context(0)
    try:
        ctx.upload(scene_a[1])
        ctx.render(_params())
        grown = jp.device_bytes_in_use()
        ctx.render(_params(16, 12))
        assert jp.device_bytes_in_use() == grown
    finally:
        ctx.close()
