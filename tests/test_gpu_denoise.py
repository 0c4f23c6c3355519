"""Guides and denoising on the MI355X: the guide buffers against jp_trace / jp_surface on camera rays rebuilt in numpy (exact), their independence
of the schedule, the filter against its numpy restatement (exact), that it denoises, no side effects, errors, and the host path."""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
import denoise_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
W, Hh = 64, 48
IMG = np.random.default_rng(3).integers(0, 256, (23, 37, 3), dtype=np.uint8)


def _arr(p, n, dt=np.float32):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy() if n else np.zeros(0, dt)


def _shape_scene(tmp_path, kind, tex, w=W, h=Hh):
    """the shape scenes of test_gpu_textures.py, rebuilt here with a w x h camera"""
    be = scenes.HostBackend("shapes")
    be.camera((0, 0, 50), (0, 0, -1), (0, 1, 0), 60.0, w, h)
    be.envlight((0, 0, 0))
    t = {"image": lambda: be.texture_image(IMG), "checker": lambda: be.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8))}[tex]()
    m = be.mat_matte(tex=t)
    rng = np.random.default_rng(11)
    if kind == "rect":
        be.rect(0, -10, 12, -8, 9, -5, False, m, None); be.rect(1, -7, 8, -9, 6, -6, False, m, None); be.rect(2, -6, 7, -5, 8, -4, True, m, None)
    elif kind == "tri":
        v = rng.uniform(-10, 10, (60, 3)).astype(f32); f = np.arange(60).reshape(20, 3)
        be.mesh(scenes.write_obj(str(tmp_path / "t.obj"), v, f, uvs=rng.uniform(-0.2, 1.2, (60, 2))), False, False, mat=m)
    elif kind == "sphere":
        be.sphere((1, -2, 0), 7.0, m, None); be.sphere((-6, 5, -3), 3.0, m, None)
    else:
        be.disk((0, 0, -2), (0.2, 0.4, 1.0), 9.0, m, None); be.disk((3, 3, 4), (-0.5, 1.0, 0.3), 4.0, m, None)
    be.preprocess()
    return be


def _upload(ctx, be, textured=True):
    ctx.upload(be.flatten(), be.flatten_textures() if textured else None)


def _guides_ref(ctx, s, w, h, seed, spp, debug=False, rows=None):
    """the definition of jp_render_guides through jp_trace and jp_surface: per sample the camera ray rebuilt in numpy, values summed in fp32 in
    sample order, scaled by 1.0f / spp.  rows: boolean mask of the rows of the shard (others 0)"""
    mat = _arr(s.prim_material, s.n_primitives, np.int32); mt = _arr(s.mat_type, s.n_materials, np.int32)
    A = np.zeros((w * h, 3), f32); N = np.zeros((w * h, 3), f32); T = np.zeros(w * h, f32)
    prims = []
    for k in range(spp):
        o, d, t0, t1 = R.camera_rays(s.camera, w, h, seed, k, debug)
        hit, t, prim, nrm = ctx.trace(o, d, t0, t1)
        prim2, _, alb = ctx.surface(o, d, t0, t1)
        assert np.array_equal(prim, prim2)
        hitb = hit != 0
        m = np.where(hitb, mat[np.maximum(prim, 0)], -1)
        coloured = hitb & (m >= 0) & np.isin(mt[np.maximum(m, 0)], [0, 1, 3])       # matte / mirror / plastic: the colour jp_surface reports
        a = np.where(coloured[:, None], alb, f32(1)).astype(f32)
        n = np.where(hitb[:, None], nrm, f32(0)).astype(f32)
        z = np.where(hitb, t, f32(0)).astype(f32)
        A = (A + a).astype(f32); N = (N + n).astype(f32); T = (T + z).astype(f32)
        prims.append(prim)
    inv = f32(1.0) / f32(spp)
    A = (A * inv).astype(f32).reshape(h, w, 3); N = (N * inv).astype(f32).reshape(h, w, 3); T = (T * inv).astype(f32).reshape(h, w)
    if rows is not None:
        A[~rows] = 0; N[~rows] = 0; T[~rows] = 0
    return A, N, T, prims


def _check_guides(ctx, be, seed=1234):
    s = be.flatten().contents
    for mode, debug in ((jp.JP_SAMPLER_COUNTER, False), (jp.JP_SAMPLER_DEBUG, True)):
        for spp in (1, 4, 7):
            rp = jp.render_params(W, Hh, 999, 0, seed, sampler_mode=mode)            # (spp and max_depth are ignored)
            alb, nrm, dep = ctx.render_guides(rp, spp)
            A, N, T, prims = _guides_ref(ctx, s, W, Hh, seed, spp, debug)
            hits = (prims[0] >= 0).mean()
            print("guides %s spp %d: hit fraction %.3f, depth mismatches %d, normal %d, albedo %d" % ("debug" if debug else "counter", spp, hits,
                  (dep != T).sum(), (nrm != N).any(-1).sum(), (alb != A).any(-1).sum()))
            assert 0.05 < hits
            assert np.array_equal(dep, T)
            assert np.array_equal(nrm, N)
            assert np.array_equal(alb, A)


# ---- 4. guides exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", ["image", "checker"])
@pytest.mark.parametrize("kind", ["rect", "tri", "sphere", "disk"])
def test_guides_exact_shape_scenes(gpu_ctx, tmp_path, kind, tex):
    be = _shape_scene(tmp_path, kind, tex)
    _upload(gpu_ctx, be)
    _check_guides(gpu_ctx, be)


def test_guides_exact_cornell(gpu_ctx):
    """full materials: the metal tall box has no colour slot -> albedo (1,1,1) there"""
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=False)
    _upload(gpu_ctx, be, textured=False)
    _check_guides(gpu_ctx, be)
    alb, _, _ = gpu_ctx.render_guides(jp.render_params(W, Hh, 1, 5, 1234), 4)
    assert (alb == 1).all(-1).mean() > 0.02          # the metal box and the light's surroundings


# ---- 5. deterministic, schedule-free, shards -------------------------------------------------------------------------------
def test_guides_deterministic_and_schedule_free(gpu_ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("t"), W, Hh, back=lambda b: b.texture_image(IMG), floor=lambda b: b.texture_checker((0.9, 0.1, 0.2), (0.1, 0.3, 0.8)))
    _upload(gpu_ctx, be)
    rp = jp.render_params(W, Hh, 1, 5, 77)
    base = gpu_ctx.render_guides(rp, 5)
    again = gpu_ctx.render_guides(rp, 5)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    try:
        for kw in (dict(lanes=1), dict(max_slots=4096), dict(blocks_per_cu=4)):
            gpu_ctx.set_options(**kw)
            got = gpu_ctx.render_guides(rp, 5)
            assert all(np.array_equal(a, b) for a, b in zip(base, got)), kw
    finally:
        gpu_ctx.set_options()
    parts = [gpu_ctx.render_guides(jp.render_params(W, Hh, 1, 5, 77, band_rows=20, shard_index=i, shard_count=2), 5) for i in range(2)]
    for k in range(3):
        assert np.array_equal((parts[0][k] + parts[1][k]).astype(f32), base[k])
        assert ((parts[0][k] != 0) & (parts[1][k] != 0)).sum() == 0
    rows = (np.arange(Hh) // 20) % 2 == 0
    assert (parts[0][2][~rows] == 0).all() and (parts[1][2][rows] == 0).all() and (parts[0][2][rows] != 0).any()
    # any of the three buffers may be NULL
    dep = np.zeros((Hh, W), f32)
    gpu_ctx._check(gpu_ctx.lib.jp_render_guides(gpu_ctx.h, C.byref(rp), 5, None, None, dep.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(dep, base[2])


# ---- 6. filter exact -------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 7), (67, 129), (256, 256), (200, 333)]                  # (H, W)
SIGMAS = [(1.0, 0.3, 0.1), (0.25, 0.1, 0.02)]


@pytest.mark.parametrize("size", SIZES)
def test_filter_bit_exact_against_numpy(size):
    ctx = jp.Context(0)                                                       # a fresh context: no scene uploaded
    try:
        h, w = size
        film, albedo, normal, depth = R.filter_inputs(h, w, 7)
        for it in range(1, 7):
            for demod in (True, False):
                for sg in SIGMAS:
                    with np.errstate(over="raise", invalid="raise", divide="raise"):
                        want = R.atrous_ref(film, albedo, normal, depth, it, *sg, demodulate=demod)
                    got = ctx.denoise(film, albedo, normal, depth, iterations=it, sigma_color=sg[0], sigma_normal=sg[1], sigma_depth=sg[2], demodulate=1 if demod else -1)
                    bad = int((got != want).any(-1).sum())
                    if bad:
                        print("filter %dx%d it %d demod %s sigma %s: %d pixels differ, max |d| %.3e" % (w, h, it, demod, sg, bad, np.abs(got - want).max()))
                    assert np.array_equal(got, want), (size, it, demod, sg)
        # the defaults: 5 iterations, sigma (1.0, 0.1, 0.03), demodulation on
        assert np.array_equal(ctx.denoise(film, albedo, normal, depth), R.atrous_ref(film, albedo, normal, depth))
        i = ctx.denoise_info()
        assert i.iterations == 5 and (i.sigma_color, i.sigma_normal, i.sigma_depth) == (f32(1.0), f32(0.1), f32(0.03)) and i.demodulated == 1 and i.denoise_ms > 0
    finally:
        ctx.close()


# ---- 7. it denoises --------------------------------------------------------------------------------------------------------
def _l2(a, b, mask=None):
    e = np.sqrt(((a.astype(np.float64) - b) ** 2).sum(-1))
    return float(e.mean() if mask is None else e[mask].mean())


def _pixel_prims(ctx, s, w, h):
    o, d, t0, t1 = R.camera_rays(s.camera, w, h, 0, 0, debug=True)
    prim, _, _ = ctx.surface(o, d, t0, t1)
    return prim.reshape(h, w)


def test_denoise_reduces_error_cornell(gpu_ctx):
    w = h = 256
    be = scenes.build_cornell(scenes.HostBackend("c"), w, h, lambert_only=False)
    _upload(gpu_ctx, be, textured=False)
    ref = gpu_ctx.render(jp.render_params(w, h, 4096, 5, 99))
    rp = jp.render_params(w, h, 16, 5, 1234)
    noisy = gpu_ctx.render(rp)
    alb, nrm, dep = gpu_ctx.render_guides(rp, 8)
    den = gpu_ctx.denoise(noisy, alb, nrm, dep)
    en, ed = _l2(noisy, ref), _l2(den, ref)
    print("cornell 256x256 16 spp: meanL2 noisy %.5f denoised %.5f ratio %.3f" % (en, ed, ed / en))
    assert ed < en


def test_denoise_reduces_error_textured_and_keeps_the_texture(gpu_ctx):
    w = h = 256
    be = scenes.build_textured_cornell(scenes.HostBackend("t"), w, h, back=lambda b: b.texture_image(IMG), floor=lambda b: b.texture_image(IMG[::-1].copy()))
    _upload(gpu_ctx, be)
    s = be.flatten().contents; t = be.flatten_textures().contents
    ref = gpu_ctx.render(jp.render_params(w, h, 4096, 5, 99))
    rp = jp.render_params(w, h, 16, 5, 1234)
    noisy = gpu_ctx.render(rp)
    alb, nrm, dep = gpu_ctx.render_guides(rp, 8)
    den = gpu_ctx.denoise(noisy, alb, nrm, dep)
    prim = _pixel_prims(gpu_ctx, s, w, h)
    mat = _arr(s.prim_material, s.n_primitives, np.int32); mtex = _arr(t.mat_texture, t.n_materials, np.int32)
    m = np.where(prim >= 0, mat[np.maximum(prim, 0)], -1)
    textured = (m >= 0) & (mtex[np.maximum(m, 0)] >= 0)
    assert 0.1 < textured.mean() < 0.9
    en, ed, tn, td = _l2(noisy, ref), _l2(den, ref), _l2(noisy, ref, textured), _l2(den, ref, textured)
    print("textured cornell 256x256 16 spp: meanL2 noisy %.5f denoised %.5f ratio %.3f; textured pixels noisy %.5f denoised %.5f ratio %.3f" % (en, ed, ed / en, tn, td, td / tn))
    assert ed < en
    assert td < tn


# ---- 8. no side effects ------------------------------------------------------------------------------------------------------
def test_guides_and_denoise_leave_the_render_alone(gpu_ctx):
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=False)
    _upload(gpu_ctx, be, textured=False)
    rp = jp.render_params(W, Hh, 8, 5, 1234)
    a = gpu_ctx.render(rp); ca = gpu_ctx.counters()
    alb, nrm, dep = gpu_ctx.render_guides(rp, 4)
    gpu_ctx.denoise(a, alb, nrm, dep)
    cm = gpu_ctx.counters()
    b = gpu_ctx.render(rp); cb = gpu_ctx.counters()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for k in ("samples", "closest_rays", "closest_hits", "shadow_rays", "shadow_occluded"):
        assert getattr(ca, k) == getattr(cb, k) == getattr(cm, k), k


def test_denoise_needs_no_scene_and_guides_do():
    ctx = jp.Context(0)
    try:
        film, albedo, normal, depth = R.filter_inputs(24, 40, 1)
        assert np.array_equal(ctx.denoise(film, albedo, normal, depth, iterations=2), R.atrous_ref(film, albedo, normal, depth, 2))
        alb = np.zeros((Hh, W, 3), f32)
        rp = jp.render_params(W, Hh, 1)
        assert ctx.lib.jp_render_guides(ctx.h, C.byref(rp), 4, alb.ctypes.data_as(C.c_void_p), None, None) == -4          # JP_ERR_NO_SCENE
    finally:
        ctx.close()


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(gpu_ctx):
    be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=True)
    _upload(gpu_ctx, be, textured=False)
    lib, hnd = gpu_ctx.lib, gpu_ctx.h
    film, albedo, normal, depth = R.filter_inputs(Hh, W, 2)
    out = np.zeros_like(film)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def dn(dp, f=film, a=albedo, n=normal, z=depth, o=out):
        return lib.jp_denoise(hnd, C.byref(dp), p(f), p(a), p(n), p(z), p(o))
    INV, UNS = -1, -5
    assert dn(jp.denoise_params(W, Hh), f=None) == INV and dn(jp.denoise_params(W, Hh), o=None) == INV
    assert dn(jp.denoise_params(W, Hh), a=None) == INV and dn(jp.denoise_params(W, Hh, demodulate=-1), a=None) == 0      # albedo: needed only to demodulate
    assert dn(jp.denoise_params(W, Hh), o=film) == INV and dn(jp.denoise_params(W, Hh), o=normal) == INV                  # out aliases an input
    big = np.zeros(2 * film.size, f32)
    assert lib.jp_denoise(hnd, C.byref(jp.denoise_params(W, Hh)), p(big[film.size // 2:]), p(albedo), p(normal), p(depth), p(big)) == INV   # ... overlaps one
    assert dn(jp.denoise_params(0, Hh)) == INV and dn(jp.denoise_params(W, -1)) == INV
    assert dn(jp.denoise_params(W, Hh, iterations=7)) == INV and dn(jp.denoise_params(W, Hh, iterations=-1)) == INV
    for bad in (-0.5, float("nan"), float("inf")):
        for k in ("sigma_color", "sigma_normal", "sigma_depth"):
            assert dn(jp.denoise_params(W, Hh, **{k: bad})) == INV, (k, bad)
    short = jp.denoise_params(W, Hh); short.struct_bytes = 12
    assert dn(short) == INV
    assert b"jp_denoise" in lib.jp_last_error()
    rp = jp.render_params(W, Hh, 1)
    g = lambda rp_, spp: lib.jp_render_guides(hnd, C.byref(rp_), spp, p(out), None, None)
    assert g(rp, 0) == INV and g(rp, 1025) == INV and g(rp, 1024) == 0
    assert g(jp.render_params(W, Hh, 1, sampler_mode=jp.JP_SAMPLER_STOCK_MT19937), 4) == UNS
    assert g(jp.render_params(W, Hh, 1, shard_index=3, shard_count=2), 4) == INV
    # ... and everything still works
    alb, nrm, dep = gpu_ctx.render_guides(rp, 2)
    assert np.array_equal(gpu_ctx.denoise(film, albedo, normal, depth, iterations=1), R.atrous_ref(film, albedo, normal, depth, 1))
    assert np.isfinite(alb).all() and (dep > 0).any()


# ---- 10. host path = C ABI path; device variants ---------------------------------------------------------------------------------
def _host_denoised(be, w, h, spp, seed, guide_spp, denoise, ldr):
    film = np.zeros((h, w, 3), f32) if ldr != 2 else None
    alb = np.zeros((h, w, 3), f32); nrm = np.zeros((h, w, 3), f32); dep = np.zeros((h, w), f32); rgb8 = np.zeros((h, w, 3), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = jp.host_lib().jp_host_render_denoised(be.h, w, h, spp, 5, seed, 0, guide_spp, denoise, ldr, p(film), p(alb), p(nrm), p(dep), p(rgb8))
    assert st == 0, st
    return film, alb, nrm, dep, rgb8


def test_host_film_requests_equal_the_c_abi_calls(gpu_ctx):
    be = scenes.build_textured_cornell(scenes.HostBackend("t"), W, Hh, back=lambda b: b.texture_image(IMG))
    _upload(gpu_ctx, be)
    rp = jp.render_params(W, Hh, 8, 5, 4321)
    noisy = gpu_ctx.render(rp)
    alb, nrm, dep = gpu_ctx.render_guides(rp, 8)
    den = gpu_ctx.denoise(noisy, alb, nrm, dep)
    assert not np.array_equal(den, noisy)
    # FFilm::RequestDenoise
    f, a, n, z, _ = _host_denoised(be, W, Hh, 8, 4321, 8, 1, 0)
    assert np.array_equal(f.view(np.uint32), den.view(np.uint32))
    assert np.array_equal(a, alb) and np.array_equal(n, nrm) and np.array_equal(z, dep)
    # FFilm::RequestGuides alone: guides, untouched film
    f, a, n, z, _ = _host_denoised(be, W, Hh, 8, 4321, 3, 0, 0)
    g3 = gpu_ctx.render_guides(rp, 3)
    assert np.array_equal(f.view(np.uint32), noisy.view(np.uint32)) and np.array_equal(a, g3[0]) and np.array_equal(n, g3[1]) and np.array_equal(z, g3[2])
    # with RequestDeviceLDR: the bytes are the existing tone map of the denoised film (the number of gamma thresholds <= x)
    thr = np.zeros(255, f32); assert gpu_ctx.lib.jp_gamma_thresholds(thr.ctypes.data_as(C.c_void_p)) == 0
    want8 = np.searchsorted(thr, den.ravel(), side="right").astype(np.uint8).reshape(Hh, W, 3)
    f, _, _, _, rgb8 = _host_denoised(be, W, Hh, 8, 4321, 8, 1, 1)
    assert np.array_equal(f.view(np.uint32), den.view(np.uint32)) and np.array_equal(rgb8, want8)
    _, _, _, _, rgb8 = _host_denoised(be, W, Hh, 8, 4321, 8, 1, 2)
    assert np.array_equal(rgb8, want8)


DEVICE_VARIANTS = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda:0")
torch.zeros(1, device=dev)                                                     # torch's runtime first, then the library's context
import jet_pbrt_amd as jp
from jet_pbrt_amd import scenes
W, Hh = 64, 48
ctx = jp.Context(0)
be = scenes.build_cornell(scenes.HostBackend("c"), W, Hh, lambert_only=False)
ctx.upload(be.flatten())
rp = jp.render_params(W, Hh, 8, 5, 1234)
noisy = ctx.render(rp)
alb, nrm, dep = ctx.render_guides(rp, 6)
den = ctx.denoise(noisy, alb, nrm, dep, iterations=4)
t_film = torch.zeros((Hh, W, 3), dtype=torch.float32, device=dev); t_alb = torch.zeros_like(t_film); t_nrm = torch.zeros_like(t_film)
t_dep = torch.zeros((Hh, W), dtype=torch.float32, device=dev); t_out = torch.zeros_like(t_film)
torch.cuda.synchronize()
ctx.render_device(rp, t_film.data_ptr(), sync=False)                           # the three stages queue up on the context stream
ctx.render_guides_device(rp, 6, t_alb.data_ptr(), t_nrm.data_ptr(), t_dep.data_ptr(), sync=False)
ctx.denoise_device(W, Hh, t_film.data_ptr(), t_alb.data_ptr(), t_nrm.data_ptr(), t_dep.data_ptr(), t_out.data_ptr(), sync=True, iterations=4)
assert np.array_equal(t_film.cpu().numpy(), noisy)
assert np.array_equal(t_alb.cpu().numpy(), alb) and np.array_equal(t_nrm.cpu().numpy(), nrm) and np.array_equal(t_dep.cpu().numpy(), dep)
assert np.array_equal(t_out.cpu().numpy(), den) and not np.array_equal(den, noisy)
try:
    ctx.denoise_device(W, Hh, t_film.data_ptr(), t_alb.data_ptr(), t_nrm.data_ptr(), t_dep.data_ptr(), t_film.data_ptr(), sync=True)
    sys.exit("out aliasing the film was accepted")
except jp.JetPbrtError:
    pass
i = ctx.denoise_info()
assert i.iterations == 4 and i.guide_spp == 6 and i.guides_ms > 0 and i.denoise_ms > 0
ctx.close()
print("DEVICE VARIANTS OK")
"""


def test_device_variants_equal_host_variants(H):
    """jp_render_device -> jp_render_guides_device -> jp_denoise_device on torch tensors give the bytes of the host variants.  In a child process,
    which brings up torch's runtime before the library's context (the order the tools use)"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", DEVICE_VARIANTS], cwd=H.REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DEVICE VARIANTS OK" in r.stdout
