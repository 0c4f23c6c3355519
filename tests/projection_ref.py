"""The camera projections (INTEGRATION.md "Projections") restated in float64 NumPy from their formulas: orthographic, equirectangular, equidistant fisheye.
Inputs are the fp32 values the library receives (camera, film positions, parameters); everything after them is float64, pi included."""
import numpy as np

import lens_ref as LR

f32 = np.float32
PERSPECTIVE, ORTHOGRAPHIC, EQUIRECT, FISHEYE = 0, 1, 2, 3
FIT_DIAGONAL, FIT_WIDTH, FIT_HEIGHT = 0, 1, 2


def axes(cam):
    """pos, right, up, front, the unit axes ex, ey, ez, and the resolution"""
    pos, front, right, up, rx, ry = LR.cam_arrays(cam)
    unit = lambda v: v / np.linalg.norm(v)
    return pos, right, up, front, unit(right), unit(up), unit(front), rx, ry


def film_ab(cam, fxfy):
    rx, ry = float(cam.res_x), float(cam.res_y)
    fxfy = np.asarray(fxfy, f32).astype(np.float64)
    return fxfy[:, 0] / rx - 0.5, 0.5 - fxfy[:, 1] / ry


def ortho_scale_of(s):
    return 1.0 if s == 0 else float(f32(s))


def fisheye_constants(cam, fov_deg, fit):
    """half the field of view in radians, and R in pixels"""
    fov = 180.0 if fov_deg == 0 else float(f32(fov_deg))
    hx, hy = float(cam.res_x) / 2.0, float(cam.res_y) / 2.0
    R = {FIT_DIAGONAL: np.hypot(hx, hy), FIT_WIDTH: hx, FIT_HEIGHT: hy}[fit]
    return np.radians(fov) / 2.0, R


def fisheye_theta(cam, fov_deg, fit, fxfy):
    half, R = fisheye_constants(cam, fov_deg, fit)
    fxfy = np.asarray(fxfy, f32).astype(np.float64)
    x = fxfy[:, 0] - float(cam.res_x) / 2.0; y = float(cam.res_y) / 2.0 - fxfy[:, 1]
    rho = np.hypot(x, y)
    return np.minimum(rho / R * half, np.pi), x, y, rho


def rays(cam, kind, fxfy, ortho_scale=0.0, fov_deg=0.0, fit=FIT_DIAGONAL):
    """origin, dir (n, 3) float64 of film positions fxfy (n, 2) under projection `kind`"""
    pos, right, up, front, ex, ey, ez, rx, ry = axes(cam)
    n = len(fxfy)
    a, b = film_ab(cam, fxfy)
    o = np.tile(pos, (n, 1))
    if kind == ORTHOGRAPHIC:
        s = ortho_scale_of(ortho_scale)
        o = pos[None] + right[None] * (a * s)[:, None] + up[None] * (b * s)[:, None]
        d = np.tile(ez, (n, 1))
    elif kind == EQUIRECT:
        phi = 2.0 * np.pi * a; th = np.pi * b
        d = ez[None] * (np.cos(th) * np.cos(phi))[:, None] + ex[None] * (np.cos(th) * np.sin(phi))[:, None] + ey[None] * np.sin(th)[:, None]
    elif kind == FISHEYE:
        th, x, y, rho = fisheye_theta(cam, fov_deg, fit, fxfy)
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(rho == 0, 0.0, np.sin(th) / rho)
        d = ez[None] * np.cos(th)[:, None] + (ex[None] * x[:, None] + ey[None] * y[:, None]) * k[:, None]
        d[rho == 0] = ez
    else:
        return LR.pinhole_rays(cam, fxfy)
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def gamma0(cam, kind, fov_deg=0.0, fit=FIT_DIAGONAL):
    """the cone spread a camera ray starts with under a projection, as the library forms it in fp32"""
    if kind == EQUIRECT:
        return f32(f32(np.pi) / f32(cam.res_y))
    if kind == FISHEYE:
        half, _ = fisheye_constants(cam, fov_deg, fit)
        hx, hy = f32(cam.res_x) / f32(2), f32(cam.res_y) / f32(2)
        R = {FIT_DIAGONAL: np.sqrt(f32(f32(hx * hx) + f32(hy * hy))), FIT_WIDTH: hx, FIT_HEIGHT: hy}[fit]
        return f32(f32(half) / f32(R))
    return f32(0)


def sample_draws(seed, x, y, s, debug=False):
    """the film positions (n, 2) of samples s of pixels (x, y): dims 0, 1 of the key; a projection draws nothing more"""
    return LR.sample_draws(seed, x, y, s, debug)[0]
