"""Synthetic scene scripts.  The reference's scene assets are not in its repository
(main.cc:34-53,94-106 read scene\\cornellbox\\*.obj and scene\\bunny\\bunny.obj), so the Cornell-box-shaped
and bunny-shaped scenes are synthesised here: geometry is written as triangulated single-mesh OBJ text
(%.9g, exact float round trip) and the scene is then created through the SAME call sequence as
main.cc:13-111 on any *backend* exposing the procedural scene API:

    camera / envlight / mat_matte / mat_mirror / mat_glass / mat_plastic / mat_metal /
    mesh / rect / sphere / preprocess

HostBackend (below) drives the product's host library; the test suite has an equivalent backend over the
compiled reference, so both sides always receive identical inputs.
"""
import ctypes as C
import hashlib
import os
import tempfile

import numpy as np

f32 = np.float32


def _fa(v):
    a = np.asarray(v, dtype=np.float32)
    return a.ctypes.data_as(C.POINTER(C.c_float)), a


def asset_dir():
    d = os.environ.get("JETPBRT_ASSET_DIR") or os.path.join(tempfile.gettempdir(), "jetpbrt_assets_%d" % os.getuid())
    os.makedirs(d, exist_ok=True)
    return d


def write_obj(path, verts, faces, uvs=None, normals=None):
    """verts (n,3) float32, faces (m,3) int 0-based -> triangulated single-mesh OBJ; uvs (n,2): `vt` per vertex, faces v/vt; normals (n,3): `vn` per
    vertex, faces v//vn (not together with uvs)."""
    verts = np.asarray(verts, np.float32)
    lines = ["o mesh"]
    lines += ["v %.9g %.9g %.9g" % (float(v[0]), float(v[1]), float(v[2])) for v in verts]
    if normals is not None:
        lines += ["vn %.9g %.9g %.9g" % (float(v[0]), float(v[1]), float(v[2])) for v in np.asarray(normals, np.float32)]
        lines += ["f %d//%d %d//%d %d//%d" % (f[0] + 1, f[0] + 1, f[1] + 1, f[1] + 1, f[2] + 1, f[2] + 1) for f in np.asarray(faces)]
    elif uvs is None:
        lines += ["f %d %d %d" % (f[0] + 1, f[1] + 1, f[2] + 1) for f in np.asarray(faces)]
    else:
        lines += ["vt %.9g %.9g" % (float(t[0]), float(t[1])) for t in np.asarray(uvs, np.float32)]
        lines += ["f %d/%d %d/%d %d/%d" % (f[0] + 1, f[0] + 1, f[1] + 1, f[1] + 1, f[2] + 1, f[2] + 1) for f in np.asarray(faces)]
    txt = "\n".join(lines) + "\n"
    tmp = path + ".tmp%d" % os.getpid()
    with open(tmp, "w") as fh:
        fh.write(txt)
    os.replace(tmp, path)
    return path


def quads_to_obj(path, quads, uv=False):
    """each quad (v0,v1,v2,v3) -> triangles (v0,v1,v2),(v0,v2,v3); uv: vertices at uv (0,0) (1,0) (1,1) (0,1)."""
    verts, faces = [], []
    for q in quads:
        b = len(verts)
        verts += [q[0], q[1], q[2], q[3]]
        faces += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    uvs = np.tile(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32), (len(quads), 1)) if uv else None
    return write_obj(path, np.array(verts, np.float32), np.array(faces), uvs)


# ---- canonical Cornell box geometry ---------------------------------------------------
CORNELL = {
    "light": [[(343, 548.7, 227), (343, 548.7, 332), (213, 548.7, 332), (213, 548.7, 227)]],
    "floor": [[(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)],
              [(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)],
              [(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]],
    "right": [[(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]],
    "left": [[(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]],
    "shortbox": [[(130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114)],
                 [(290, 0, 114), (290, 165, 114), (240, 165, 272), (240, 0, 272)],
                 [(130, 0, 65), (130, 165, 65), (290, 165, 114), (290, 0, 114)],
                 [(82, 0, 225), (82, 165, 225), (130, 165, 65), (130, 0, 65)],
                 [(240, 0, 272), (240, 165, 272), (82, 165, 225), (82, 0, 225)]],
    "tallbox": [[(423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)],
                [(423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)],
                [(472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)],
                [(314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)],
                [(265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247)]],
}


def light_radiance():
    """main.cc:35: 8*(0.747+0.058, 0.747+0.258, 0.747) + 15.6*(...) + 18.4*(...), in fp32."""
    def v(a, b, c):
        return np.array([f32(a), f32(b), f32(c)], np.float32)
    r = (f32(8.0) * v(f32(0.747) + f32(0.058), f32(0.747) + f32(0.258), 0.747)
         + f32(15.6) * v(f32(0.740) + f32(0.287), f32(0.740) + f32(0.160), 0.740)
         + f32(18.4) * v(f32(0.737) + f32(0.642), f32(0.737) + f32(0.159), 0.737))
    return r.astype(np.float32)


def _normalize(v):
    v = np.asarray(v, np.float32)
    l2 = f32(v[0] * v[0]) + f32(v[1] * v[1])
    l2 = f32(l2) + f32(v[2] * v[2])
    ln = np.sqrt(f32(l2), dtype=np.float32)
    return (v / ln).astype(np.float32)


def cornell_assets():
    d = asset_dir()
    out = {}
    for name, quads in CORNELL.items():
        p = os.path.join(d, "cornell_%s.obj" % name)
        if not os.path.exists(p):
            quads_to_obj(p, quads)
        out[name] = p
    return out


def bunny_mesh(n_lon=187, n_lat=188):
    """Deterministic bunny-shaped stand-in for scene\\bunny\\bunny.obj (not in the reference repository): a closed
    displaced sphere (body + head + two ears) in the bunny's native scale -- about 0.15 units tall, resting
    near y = 0.03 -- with 2*n_lon*(n_lat-1) triangles (69,938 at the defaults)."""
    th = (np.arange(1, n_lat, dtype=np.float64) / n_lat) * np.pi          # interior latitudes
    ph = (np.arange(n_lon, dtype=np.float64) / n_lon) * 2.0 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")

    def dirs(t, p):
        return np.stack([np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)], -1)

    def radius(d):
        r = 0.055 + 0.0 * d[..., 0]
        lobes = [((0.55, 0.80, 0.0), 0.030, 10.0),      # head
                 ((0.45, 0.95, 0.22), 0.060, 60.0),     # ear
                 ((0.45, 0.95, -0.22), 0.060, 60.0),    # ear
                 ((-0.9, -0.2, 0.0), 0.020, 12.0),      # tail
                 ((0.0, -1.0, 0.0), -0.012, 3.0)]       # flattened base
        for c, amp, sharp in lobes:
            c = np.array(c) / np.linalg.norm(c)
            r = r + amp * np.exp(sharp * (d @ c - 1.0))
        r = r + 0.0015 * np.sin(14 * d[..., 0] * np.pi) * np.sin(11 * d[..., 2] * np.pi) * np.sin(9 * d[..., 1] * np.pi)  # fur-scale detail
        return r

    D = dirs(T, P)
    V = D * radius(D)[..., None]
    top = np.array([0.0, 1.0, 0.0]); bot = np.array([0.0, -1.0, 0.0])
    vt = top * radius(top[None])[0]; vb = bot * radius(bot[None])[0]
    verts = np.concatenate([V.reshape(-1, 3), vt[None], vb[None]], 0)
    verts[:, 1] += 0.1                                                  # centre at y = 0.1
    nring = n_lat - 1
    it, ib = nring * n_lon, nring * n_lon + 1
    faces = []
    idx = lambda i, j: i * n_lon + (j % n_lon)
    for j in range(n_lon):
        faces.append((it, idx(0, j + 1), idx(0, j)))
        faces.append((ib, idx(nring - 1, j), idx(nring - 1, j + 1)))
    i = np.arange(nring - 1)[:, None]; j = np.arange(n_lon)[None, :]
    a = i * n_lon + j; b = i * n_lon + (j + 1) % n_lon; c = (i + 1) * n_lon + j; e = (i + 1) * n_lon + (j + 1) % n_lon
    quads = np.stack([np.stack([a, b, e], -1), np.stack([a, e, c], -1)], -2).reshape(-1, 3)
    faces = np.concatenate([np.array(faces, np.int64), quads], 0)
    return verts.astype(np.float32), faces


def bunny_asset(n_lon=187, n_lat=188):
    p = os.path.join(asset_dir(), "bunny_%dx%d.obj" % (n_lon, n_lat))
    if not os.path.exists(p):
        v, f = bunny_mesh(n_lon, n_lat)
        write_obj(p, v, f)
    return p


def file_sha1(path):
    h = hashlib.sha1()
    with open(path, "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()


# ---- backend over the product's host library ------------------------------------------------------------------
class HostBackend:
    prefix = "jp_host_"

    def __init__(self, name="scene", lib=None):
        if lib is None:
            from . import host_lib
            lib = host_lib()
        self.L = lib
        self._new(name)

    def _new(self, name):
        self.h = C.c_void_p(self.L.jp_host_scene_new(name.encode()))

    def _f(self, n):
        return getattr(self.L, self.prefix + n)

    def camera(self, lookfrom, front, up, vfov, resx, resy):
        a, _a = _fa(lookfrom); b, _b = _fa(front); c, _c = _fa(up)
        self._f("scene_camera")(self.h, a, b, c, C.c_float(vfov), C.c_float(resx), C.c_float(resy))

    def envlight(self, rgb):
        a, _a = _fa(rgb); return self._f("scene_envlight")(self.h, a)

    def pointlight(self, pos, intensity):
        a, _a = _fa(pos); b, _b = _fa(intensity); return self._f("scene_pointlight")(self.h, a, b)

    def dirlight(self, direction, irradiance):
        a, _a = _fa(direction); b, _b = _fa(irradiance); return self._f("scene_dirlight")(self.h, a, b)

    def mat_matte(self, rgb=None, tex=None):
        if tex is not None:
            return self._f("mat_matte_tex")(self.h, tex)
        a, _a = _fa(rgb); return self._f("mat_matte")(self.h, a)

    def mat_mirror(self, rgb=None, tex=None):
        if tex is not None:
            return self._f("mat_mirror_tex")(self.h, tex)
        a, _a = _fa(rgb); return self._f("mat_mirror")(self.h, a)

    # textures (host backend only): handles for the tex= argument of mat_matte / mat_mirror / mat_plastic
    def texture_solid(self, rgb):
        a, _a = _fa(rgb); return self._f("texture_solid")(self.h, a)

    def texture_checker(self, odd, even):
        a, _a = _fa(odd); b, _b = _fa(even); return self._f("texture_checker")(self.h, a, b)

    def texture_image(self, rgb8, sampling=None):
        """rgb8: (H, W, 3) uint8, top row first; sampling: a JpTexSampler (jet_pbrt_amd.tex_sampler), FImageTexture::SetSampling"""
        img = np.ascontiguousarray(rgb8, np.uint8)
        k = self._f("texture_image")(self.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0])
        if sampling is not None:
            self.texture_set_sampling(k, sampling)
        return k

    def texture_set_sampling(self, tex, sampling):
        """FImageTexture::SetSampling (None: no record of its own)"""
        if self._f("texture_set_sampling")(self.h, tex, None if sampling is None else C.byref(sampling)) != 0:
            raise RuntimeError("texture_set_sampling failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def normal_map_set_sampling(self, nmap, sampling):
        """FNormalMap::SetSampling (None: no record of its own)"""
        if self._f("normal_map_set_sampling")(self.h, nmap, None if sampling is None else C.byref(sampling)) != 0:
            raise RuntimeError("normal_map_set_sampling failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def set_texture_sampling_default(self, sampling):
        """FScene::SetTextureSamplingDefault: the record of every image texture without one of its own (None: the identity)"""
        self._f("scene_set_texture_sampling_default")(self.h, None if sampling is None else C.byref(sampling))

    def flatten_texture_sampling(self):
        """the scene's sampling records as a JpTextureSampling for Context.set_texture_sampling (None: every record is the identity); valid until the next preprocess"""
        p = self.L.jp_host_flatten_texture_sampling(self.h)
        return p.contents if p else None

    def texture_set_mipmaps(self, tex, on):
        """FImageTexture::SetMipmaps (None: the scene's default)"""
        if self._f("texture_set_mipmaps")(self.h, tex, -1 if on is None else int(bool(on))) != 0:
            raise RuntimeError("texture_set_mipmaps failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def set_texture_mipmap_default(self, on=True, footprint_scale=0.0, bounce_spread=0.0):
        """FScene::SetTextureMipmapDefault: mip maps for every image texture without a choice of its own, and the scene's footprint scale and bounce spread (0: defaults)"""
        self._f("scene_set_texture_mipmap_default")(self.h, int(bool(on)), C.c_float(footprint_scale), C.c_float(bounce_spread))

    def flatten_texture_mipmaps(self):
        """the scene's mipmap modes as a JpTextureMipmaps for Context.set_texture_mipmaps (None: every mode is OFF); valid until the next preprocess"""
        p = self.L.jp_host_flatten_texture_mipmaps(self.h)
        return p.contents if p else None

    def texture_procedural(self, record, odd, even):
        """FProceduralTexture from a JpProcedural (jp.procedural(...)): the colour at t = 1 (odd) and at t = 0 (even); flattens as their CHECKER plus the record"""
        a, _a = _fa(odd); b, _b = _fa(even)
        k = self._f("texture_procedural")(self.h, C.byref(record), a, b)
        if k < 0:
            raise RuntimeError("texture_procedural failed: %s" % self.L.jp_host_last_error(self.h).decode())
        return k

    def flatten_texture_procedurals(self):
        """the scene's procedural records as a JpTextureProcedurals for Context.set_texture_procedurals (None: no record); valid until the next preprocess"""
        p = self.L.jp_host_flatten_texture_procedurals(self.h)
        return p.contents if p else None

    def normal_map_from_procedural(self, record, w, h, scale):
        """FNormalMap::FromProcedural: a w x h height image baked from the record with the host lookup, then FromHeight -> normal map index"""
        k = self._f("normal_map_from_procedural")(self.h, C.byref(record), int(w), int(h), C.c_float(scale))
        if k < 0:
            raise RuntimeError("normal_map_from_procedural failed: %s" % self.L.jp_host_last_error(self.h).decode())
        return k

    def texture_image_file(self, path):
        """FImageTexture(filename): binary PPM or uncompressed BMP; anything else is the reference's solid cyan"""
        return self._f("texture_image_file")(self.h, path.encode())

    def mat_set_texture(self, mat, tex):
        """FMaterial::texture of any material (flatten refuses one on glass / metal)"""
        return self._f("mat_set_texture")(self.h, mat, tex)

    def flatten_textures(self):
        p = self.L.jp_host_flatten_textures(self.h)
        if not p:
            raise RuntimeError("flatten failed: %s" % self.L.jp_host_last_error(self.h).decode())
        return p

    def mat_glass(self, eta, kr, kt):
        a, _a = _fa(kr); b, _b = _fa(kt); return self._f("mat_glass")(self.h, C.c_float(eta), a, b)

    def mat_plastic(self, kd, ks, rough, remap=False, tex=None):
        b, _b = _fa(ks)
        if tex is not None:
            return self._f("mat_plastic_tex")(self.h, tex, b, C.c_float(rough), int(remap))
        a, _a = _fa(kd); return self._f("mat_plastic")(self.h, a, b, C.c_float(rough), int(remap))

    def mat_metal(self, eta, k, ur, vr, remap=False):
        a, _a = _fa(eta); b, _b = _fa(k); return self._f("mat_metal")(self.h, a, b, C.c_float(ur), C.c_float(vr), int(remap))

    def mesh(self, path, flip_normal, flip_hand, offset=(0, 0, 0), scale=1.0, mat=-1, radiance=None, smooth=None):
        """smooth (host backend only): None flat (as ever, even when the file has vn), "file" the file's vn, a number: normals computed with that crease angle in degrees"""
        o, _o = _fa(offset)
        r, _r = _fa(radiance) if radiance is not None else (None, None)
        if smooth is not None:
            mode, angle = (1, 0.0) if smooth == "file" else (2, float(smooth))
            return self._f("scene_mesh_smooth")(self.h, path.encode(), int(flip_normal), int(flip_hand), o, C.c_float(scale), mat, r, mode, C.c_float(angle))
        return self._f("scene_mesh")(self.h, path.encode(), int(flip_normal), int(flip_hand), o, C.c_float(scale), mat, r)

    def rect(self, axis, a0, a1, b0, b1, c, flip=False, mat=-1, radiance=None):
        r, _r = _fa(radiance) if radiance is not None else (None, None)
        self._f("scene_rect")(self.h, axis, C.c_float(a0), C.c_float(a1), C.c_float(b0), C.c_float(b1), C.c_float(c), int(flip), mat, r)

    def sphere(self, center, radius, mat=-1, radiance=None):
        cc, _c = _fa(center)
        r, _r = _fa(radiance) if radiance is not None else (None, None)
        self._f("scene_sphere")(self.h, cc, C.c_float(radius), mat, r)

    def disk(self, pos, normal, radius, mat=-1, radiance=None):
        pp, _p = _fa(pos); nn, _n = _fa(normal)
        r, _r = _fa(radiance) if radiance is not None else (None, None)
        self._f("scene_disk")(self.h, pp, nn, C.c_float(radius), mat, r)

    def preprocess(self):
        self._f("scene_preprocess")(self.h)

    def set_reference_tree(self, on=True, certified=False):
        """FScene::referenceTree: build the reference's own tree (its rand() sequence, its std::sort) and have the device
        walk it with the reference's semantics -- bit-identical hits on meshes, several times slower (host backend only).
        certified=True (FScene::certifiedWalk): the certified walk over that tree's leaves, about twice as fast; proven identical ray
        by ray except for secondary rays within fp32 noise of a triangle's plane (about one in 10^9; a generous cull slack reaches those seen: the 280k-triangle frames measured are bit-identical)."""
        self._f("scene_set_reference_tree")(self.h, (2 if certified else 1) if on else 0)

    def set_light_sampling(self, mode="power"):
        """FScene::SetLightSampling: "power" = one light per bounce picked by power (JP_LIGHTS_POWER_ONE, emissive meshes of any size),
        None / "all" = every light at every bounce (host backend only; takes effect with the integrator's next upload)"""
        from . import LIGHT_SAMPLING_MODES
        self._f("scene_set_light_sampling")(self.h, LIGHT_SAMPLING_MODES[mode])

    def set_estimator(self, mode="mis"):
        """FScene::SetEstimator: "mis" = next-event estimation and the BSDF sample weighted against each other (JP_ESTIMATOR_MIS; the scene is then
        uploaded with JP_LIGHTS_POWER_ONE), None / "nee" = the reference's estimator (host backend only; takes effect with the integrator's next render)"""
        from . import ESTIMATOR_MODES
        self._f("scene_set_estimator")(self.h, ESTIMATOR_MODES[mode])

    def set_lens(self, radius, focus=1.0, blades=0, rotation=0.0, focus_at=None):
        """FCamera::SetLens on the scene's camera: a thin lens of `radius` scene units focused at distance `focus` (blades 0: a disk, 3 .. 16: a polygon turned by
        `rotation` degrees); focus_at=(fx, fy): FCamera::FocusAt, the focus distance is found at render time from what that film position sees (last_focus() tells it).
        radius 0: the pinhole again (host backend only; takes effect with the integrator's next render)"""
        fx, fy = focus_at if focus_at is not None else (0.0, 0.0)
        if self._f("scene_set_lens")(self.h, C.c_float(radius), C.c_float(focus), int(blades), C.c_float(rotation), 0 if focus_at is None else 1, C.c_float(fx), C.c_float(fy)) != 0:
            raise RuntimeError("set_lens failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def set_projection(self, kind, ortho_scale=0.0, fov_deg=0.0, fit="diagonal"):
        """FCamera::SetProjection on the scene's camera: "ortho", "equirect", "fisheye" or "perspective" (or JP_PROJ_*), validated by the library's
        jp_check_projection (host backend only; takes effect with the integrator's next render)"""
        from . import PROJECTIONS, FITS
        k = PROJECTIONS[kind] if isinstance(kind, str) else int(kind)
        f = FITS[fit] if isinstance(fit, str) else int(fit)
        if self._f("scene_set_projection")(self.h, k, C.c_float(ortho_scale), C.c_float(fov_deg), f) != 0:
            raise RuntimeError("set_projection failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def last_focus(self):
        """FCamera::LastFocus: the focus distance of the last render with a lens"""
        return float(self.L.jp_host_last_focus(self.h))

    def envmap(self, rgb, up_axis="z", importance=0):
        """FScene::SetEnvironmentMap: an (H, W, 3) float32 array top row first, the path of a PFM / Radiance .hdr / binary PPM / BMP file, or None for no
        map; up_axis "z" (map space = world space) or "y"; importance -1: sample by solid angle alone, arrays only (host backend only; takes effect
        with the integrator's next upload).  The scene's one envlight() tints the map."""
        from . import ENV_UP_AXES
        if rgb is None:
            st = self._f("scene_envmap")(self.h, None, 0, 0, 0, 0)
        elif isinstance(rgb, (str, bytes, os.PathLike)):
            st = self._f("scene_envmap_file")(self.h, os.fsencode(rgb), ENV_UP_AXES[up_axis])
        else:
            a = np.ascontiguousarray(rgb, np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise RuntimeError("an environment map is an (H, W, 3) array")
            st = self._f("scene_envmap")(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], ENV_UP_AXES[up_axis], importance)
        if st != 0:
            raise RuntimeError("envmap failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def flatten_normals(self):
        """the scene's vertex normals as a JpVertexNormals for Context.set_vertex_normals (None: no smooth triangle); valid until the next preprocess"""
        p = self.L.jp_host_flatten_normals(self.h)
        return p.contents if p else None

    # normal maps (host backend only): handles for mat_set_normal_map
    def _nmap(self, k, what):
        if k < 0:
            raise RuntimeError("%s failed: %s" % (what, self.L.jp_host_last_error(self.h).decode()))
        return k

    def normal_map(self, rgb8, sampling=None):
        """FNormalMap from memory: (H, W, 3) uint8, top row first; or the path of a binary PPM / BMP file (FNormalMap::FromFile); sampling: a JpTexSampler
        (FNormalMap::SetSampling)"""
        if isinstance(rgb8, (str, bytes, os.PathLike)):
            k = self._nmap(self._f("normal_map_file")(self.h, os.fsencode(rgb8)), "normal_map")
        else:
            img = np.ascontiguousarray(rgb8, np.uint8)
            if img.ndim != 3 or img.shape[2] != 3:
                raise RuntimeError("a normal map is an (H, W, 3) uint8 array")
            k = self._nmap(self._f("normal_map")(self.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0]), "normal_map")
        if sampling is not None:
            self.normal_map_set_sampling(k, sampling)
        return k

    def normal_map_from_height(self, grey, scale):
        """FNormalMap::FromHeight: (H, W) uint8 heights, top row first -> the map of their slopes times `scale`"""
        img = np.ascontiguousarray(grey, np.uint8)
        if img.ndim != 2:
            raise RuntimeError("a height map is an (H, W) uint8 array")
        return self._nmap(self._f("normal_map_from_height")(self.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], C.c_float(scale)), "normal_map_from_height")

    def normal_map_data(self, nmap):
        """the map's texels, (H, W, 3) uint8"""
        w = C.c_int(0); h = C.c_int(0)
        if self._f("normal_map_read")(self.h, nmap, C.byref(w), C.byref(h), None) != 0:
            raise RuntimeError("normal_map_data failed: %s" % self.L.jp_host_last_error(self.h).decode())
        out = np.zeros((h.value, w.value, 3), np.uint8)
        self._f("normal_map_read")(self.h, nmap, None, None, out.ctypes.data_as(C.c_void_p))
        return out

    def mat_set_normal_map(self, mat, nmap, strength=1.0):
        """FMaterial::normalMap / normalStrength of any material (nmap -1 or None: none)"""
        if self._f("mat_set_normal_map")(self.h, mat, -1 if nmap is None else nmap, C.c_float(strength)) != 0:
            raise RuntimeError("mat_set_normal_map failed: %s" % self.L.jp_host_last_error(self.h).decode())

    def flatten_normal_maps(self):
        """the scene's normal maps as a JpNormalMaps for Context.set_normal_maps (None: no material carries one); valid until the next preprocess"""
        p = self.L.jp_host_flatten_normal_maps(self.h)
        return p.contents if p else None

    def flatten_envmap(self):
        """the scene's map as a JpEnvMap pointer for Context.set_environment_map (None: no map); valid until the map changes"""
        p = self.L.jp_host_flatten_envmap(self.h)
        return p.contents if p else None

    def set_device_build(self, on=True):
        """FScene::deviceBuild: leave the hierarchy to jp_upload_scene's device LBVH pass (host backend only)."""
        self._f("scene_set_device_build")(self.h, 1 if on else 0)

    def num_primitives(self):
        return self._f("num_primitives")(self.h)

    def num_lights(self):
        return self._f("num_lights")(self.h)

    # host-only
    def flatten(self):
        p = self.L.jp_host_flatten(self.h)
        if not p:
            raise RuntimeError("flatten failed: %s" % self.L.jp_host_last_error(self.h).decode())
        return p

    def close(self):
        if self.h:
            self._f("scene_free")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AXIS_XY, AXIS_XZ, AXIS_YZ = 0, 1, 2


# ---- scene scripts (the calls of main.cc) -----------------------------------------------------------------------
def build_cornell(be, width, height, lambert_only=False, extras=None, env=(0.0, 0.0, 0.0)):
    """create_cornellbox_scene main.cc:13-62.  lambert_only swaps the metal tall box for white matte (config C2)."""
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    be.camera(lookfrom, _normalize(lookat - lookfrom), (0, 1, 0), 60.0, width, height)
    be.envlight(env)
    red = be.mat_matte((0.63, 0.065, 0.05))
    green = be.mat_matte((0.14, 0.45, 0.091))
    white = be.mat_matte((0.725, 0.71, 0.68))
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    A = cornell_assets()
    be.mesh(A["light"], True, True, mat=mat_light, radiance=light_radiance())
    be.mesh(A["floor"], True, True, mat=white)
    be.mesh(A["shortbox"], True, True, mat=white)
    be.mesh(A["tallbox"], True, True, mat=(white if lambert_only else golden))
    be.mesh(A["left"], True, True, mat=red)
    be.mesh(A["right"], True, True, mat=green)
    if extras:
        extras(be, dict(red=red, green=green, white=white, golden=golden))
    be.preprocess()
    return be


def cornell_textured_assets():
    """the Cornell box with the floor / ceiling / back wall as three meshes, each with uv (0,0) (1,0) (1,1) (0,1) at its corners"""
    d = asset_dir()
    out = {}
    for name, quads in (("floor_only", CORNELL["floor"][:1]), ("ceiling", CORNELL["floor"][1:2]), ("back", CORNELL["floor"][2:3])):
        p = os.path.join(d, "cornell_uv_%s.obj" % name)
        if not os.path.exists(p):
            quads_to_obj(p, quads, uv=True)
        out[name] = p
    return out


def build_textured_cornell(be, width, height, back=None, left=None, right=None, floor=None, full_materials=True, mirror=None, plastic=None):
    """The Cornell box of build_cornell with texture-mapped materials (HostBackend only).  back / left / right / floor: a callable
    be -> texture handle for the matte back wall, red wall, green wall, floor; an rgb triple (a constant colour instead of the usual one);
    None (the usual colour).  full_materials adds the metal tall box and a mirror and a plastic sphere, whose specularColor / Kd take
    `mirror` / `plastic` the same way."""
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    be.camera(lookfrom, _normalize(lookat - lookfrom), (0, 1, 0), 60.0, width, height)
    be.envlight((0.0, 0.0, 0.0))
    def matte(rgb, tex):
        if callable(tex):
            return be.mat_matte(tex=tex(be))
        return be.mat_matte(rgb if tex is None else tex)
    red = matte((0.63, 0.065, 0.05), left)
    green = matte((0.14, 0.45, 0.091), right)
    white = be.mat_matte((0.725, 0.71, 0.68))
    wall = matte((0.725, 0.71, 0.68), back)
    ground = matte((0.725, 0.71, 0.68), floor)
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    A = cornell_assets(); T = cornell_textured_assets()
    be.mesh(A["light"], True, True, mat=mat_light, radiance=light_radiance())
    be.mesh(T["floor_only"], True, True, mat=ground)
    be.mesh(T["ceiling"], True, True, mat=white)
    be.mesh(T["back"], True, True, mat=wall)
    be.mesh(A["shortbox"], True, True, mat=white)
    be.mesh(A["tallbox"], True, True, mat=(golden if full_materials else white))
    be.mesh(A["left"], True, True, mat=red)
    be.mesh(A["right"], True, True, mat=green)
    if full_materials:
        mm = be.mat_mirror(tex=mirror(be)) if callable(mirror) else be.mat_mirror((0.9, 0.9, 0.9) if mirror is None else mirror)
        ks = (0.3, 0.25, 0.2)
        pm = be.mat_plastic(None, ks, 0.3, True, tex=plastic(be)) if callable(plastic) else be.mat_plastic((0.35, 0.12, 0.48) if plastic is None else plastic, ks, 0.3, True)
        be.sphere((120, 330, -300), 40.0, mm, None)
        be.sphere((420, 90, -120), 50.0, pm, None)
    be.preprocess()
    return be


# ---- mesh lights (INTEGRATION.md "Light selection") ----------------------------------------------------------------
LAMP_RECT = (213.0, 343.0, 227.0, 332.0, 548.7)      # the Cornell box's ceiling light: x0, x1, z0, z1 (OBJ handedness), y


def lamp_grid_asset(nx, nz, rect=LAMP_RECT, warp=0.0, name=None):
    """A rectangle of the ceiling plane as nx x nz quads (2 nx nz triangles, wound like cornellbox/light.obj: facing down when loaded with
    flip_normal and flip_handedness).  warp 0: a regular grid (equal triangles, the tessellated rectangle light); warp > 0: the grid lines are
    spaced unevenly (triangle areas differ by up to (1 + warp)^2 : (1 - warp)^2 and more)."""
    x0, x1, z0, z1, y = rect
    def cuts(a, b, n, phase):
        t = np.arange(n + 1, dtype=np.float64) / n
        t = t + warp * np.sin(np.pi * t) * np.cos(2.5 * np.pi * t + phase) / 2.0 if warp else t
        t = np.sort(np.clip(t, 0.0, 1.0)); t[0], t[-1] = 0.0, 1.0
        return (a + (b - a) * t).astype(np.float32)
    xs, zs = cuts(x0, x1, nx, 0.3), cuts(z0, z1, nz, 1.1)
    quads = [[(xs[i + 1], y, zs[j]), (xs[i + 1], y, zs[j + 1]), (xs[i], y, zs[j + 1]), (xs[i], y, zs[j])] for i in range(nx) for j in range(nz)]
    p = os.path.join(asset_dir(), name or "lamp_%dx%d_%g_%s.obj" % (nx, nz, warp, hashlib.sha1(repr(rect).encode()).hexdigest()[:8]))
    if not os.path.exists(p):
        quads_to_obj(p, quads)
    return p


def build_lamp_box(be, width, height, lamp, floor=None, full_materials=False):
    """The Cornell box WITHOUT its light and without an environment light: `lamp(be, mats)` creates every light of the scene, in its own order
    (mats: white / light material indices).  floor: as build_textured_cornell takes it (a texture on the floor)."""
    lookfrom = np.array([278, 273, 960], np.float32); lookat = np.array([278, 273, 0], np.float32)
    be.camera(lookfrom, _normalize(lookat - lookfrom), (0, 1, 0), 60.0, width, height)
    red = be.mat_matte((0.63, 0.065, 0.05))
    green = be.mat_matte((0.14, 0.45, 0.091))
    white = be.mat_matte((0.725, 0.71, 0.68))
    ground = be.mat_matte(tex=floor(be)) if callable(floor) else be.mat_matte((0.725, 0.71, 0.68) if floor is None else floor)
    golden = be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False)
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    A = cornell_assets(); T = cornell_textured_assets()
    lamp(be, dict(white=white, light=mat_light))
    be.mesh(T["floor_only"], True, True, mat=ground)
    be.mesh(T["ceiling"], True, True, mat=white)
    be.mesh(T["back"], True, True, mat=white)
    be.mesh(A["shortbox"], True, True, mat=white)
    be.mesh(A["tallbox"], True, True, mat=(golden if full_materials else white))
    be.mesh(A["left"], True, True, mat=red)
    be.mesh(A["right"], True, True, mat=green)
    be.preprocess()
    return be


def lamp_rect(radiance=None, rect=LAMP_RECT):
    """the ceiling light as ONE rectangle light (facing down)"""
    def lamp(be, m):
        x0, x1, z0, z1, y = rect
        be.rect(AXIS_XZ, x0, x1, -z1, -z0, y, True, m["light"], light_radiance() if radiance is None else radiance)
    return lamp


def lamp_mesh(nx, nz, radiance=None, rect=LAMP_RECT, warp=0.0):
    """the ceiling light as an emissive mesh of 2 nx nz triangles, every one an FAreaLight (FScene::CreateAreaLights)"""
    def lamp(be, m):
        be.mesh(lamp_grid_asset(nx, nz, rect, warp), True, True, mat=m["light"], radiance=light_radiance() if radiance is None else radiance)
    return lamp


def lamp_66(be, m):
    """66 lights: two rectangle lights of different radiance and size, then a 64-triangle emissive mesh (8 x 4 quads) of unequal triangles"""
    be.rect(AXIS_XZ, 60.0, 150.0, -180.0, -110.0, 548.7, True, m["light"], (30.0, 24.0, 18.0))
    be.rect(AXIS_XZ, 420.0, 480.0, -460.0, -400.0, 548.7, True, m["light"], (8.0, 12.0, 20.0))
    lamp_mesh(8, 4, (12.0, 11.0, 9.0), (200.0, 360.0, 240.0, 320.0, 548.7), warp=0.6)(be, m)


def build_bunny(be, width, height, n_lon=187, n_lat=188, instances=4, obj_path=None, smooth=None):
    """create_bunny_scene main.cc:64-111 with the procedural stand-in mesh (4 instances as in the reference); smooth: HostBackend.mesh's (host backend only)."""
    lookfrom = np.array([-300, 300, -300], np.float32); lookat = np.array([0, 0, 0], np.float32)
    be.camera(lookfrom, _normalize(lookat - lookfrom), (0, 1, 0), 60.0, width, height)
    be.envlight((0.1, 0.1, 0.5))
    red = be.mat_matte((0.63, 0.065, 0.05))
    green = be.mat_matte((0.14, 0.45, 0.091))
    be.mat_matte((0.725, 0.71, 0.68))
    mat_light = be.mat_matte((0.65, 0.65, 0.65))
    be.rect(AXIS_XZ, -100, 100, -100, 100, 350, True, mat_light, light_radiance())
    be.rect(AXIS_XZ, -200, 200, -200, 200, 0, False, green, None)
    obj = obj_path or bunny_asset(n_lon, n_lat)
    kd = np.array([0.35, 0.12, 0.48], np.float32)
    mats = [lambda: red,
            lambda: be.mat_plastic(kd, (np.float32(1) - kd).astype(np.float32), 0.1, False),
            lambda: be.mat_metal((0.18, 0.15, 0.81), (0.11, 0.11, 0.11), 0.2, 0.2, False),
            lambda: be.mat_glass(1.5, (0.98, 0.98, 0.98), (0.98, 0.98, 0.98))]
    offsets = [(0, 0, 0), (-100, 0, -100), (0, 0, -100), (-100, 0, 0)]
    for i in range(instances):
        if smooth is None:
            be.mesh(obj, True, True, offsets[i], 500.0, mats[i](), None)
        else:
            be.mesh(obj, True, True, offsets[i], 500.0, mats[i](), None, smooth=smooth)
    be.preprocess()
    return be


def build_misc(be, width, height):
    """Coverage scene for API paths no benchmark scene reaches: FSphere as primitive and as area light
    (shape.h:476-662), FMirrorMaterial, glass sphere (the commented-out one of main.cc:56-58), remapped
    roughness, a null-material primitive (integrator.cc:349-353) and a non-black environment."""
    def extras(b, m):
        glass = b.mat_glass(1.5, (0.98, 0.98, 0.98), (0.98, 0.98, 0.98))
        mirror = b.mat_mirror((0.9, 0.9, 0.9))
        plastic = b.mat_plastic((0.35, 0.12, 0.48), (0.3, 0.3, 0.3), 0.3, True)
        b.sphere((273, 273, 150), 60.0, glass, None)
        b.sphere((120, 330, 300), 40.0, mirror, None)
        b.sphere((420, 90, 120), 50.0, plastic, None)
        b.sphere((278, 440, 280), 25.0, m["white"], (np.array([20, 16, 12], np.float32)))
        b.rect(AXIS_XY, 150, 400, 100, 400, 500, False, -1, None)          # null material: rays pass through
    be_ = build_cornell(be, width, height, lambert_only=False, extras=extras, env=(0.05, 0.08, 0.2))
    return be_


def build_lights(be, width, height):
    """Cornell box lit additionally by the delta lights of light.h:81-180 (FPointLight, FDirectionLight -- only in
    commented-out lines of main.cc:38,82) and a dim environment."""
    def extras(b, m):
        b.pointlight((278, 273, -200), (630000.0 * 0.2, 650000.0 * 0.2, 650000.0 * 0.2))
        b.dirlight((0.3, -1.0, -0.6), (1.5, 1.2, 0.9))
    return build_cornell(be, width, height, lambert_only=False, extras=extras, env=(0.02, 0.02, 0.05))


def build_disks(be, width, height):
    """Cornell box with FDisk shapes (shape.h:189-275; no configuration of main.cc creates one): a disk area light below the
    ceiling, tilted matte / metal / glass disks as occluders, a disk parallel to an axis-aligned wall, a tiny and a large one."""
    def extras(b, m):
        b.disk((278, 540, -279.5), (0.0, -1.0, 0.0), 60.0, m["white"], (17.0, 12.0, 4.0))       # a second, round light, facing down
        b.disk((150, 120, -200), (0.3, 0.8, 0.5), 70.0, m["white"], None)
        metal = b.mat_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.15, 0.3, False)
        b.disk((400, 200, -350), (-0.6, 0.5, 0.7), 90.0, metal, None)
        glass = b.mat_glass(1.5, (0.98, 0.98, 0.98), (0.98, 0.98, 0.98))
        b.disk((278, 300, -150), (0.1, 0.2, 1.0), 55.0, glass, None)
        b.disk((1.0, 274, -280), (1.0, 0.0, 0.0), 100.0, m["white"], None)                        # just in front of the left wall
        b.disk((300, 1.5, -100), (0.0, 1.0, 0.0), 3.0, metal, None)
    return build_cornell(be, width, height, lambert_only=False, extras=extras, env=(0.03, 0.03, 0.03))


PROCEDURAL_VIEWS = {"near": ((0, 3, 0), (0.0, -1.0, -0.35), (0, 0, -1)), "far": ((0, 3, 0), (0.0, -0.06, -1.0), (0, 1, 0))}


def build_procedural_floor(be, width, height, record=None, view="far"):
    """A floor to the horizon under a white sky, for the tools: `record` (a JpProcedural; None: the plain checker) on the floor's texture, seen from 3 units above --
    "near": looking down, every octave in reach; "far": looking along it, the ray cone's footprint swallowing octave after octave."""
    pos, front, up = PROCEDURAL_VIEWS[view]
    be.camera(pos, _normalize(np.array(front, np.float32)), up, 50.0, width, height)
    be.envlight((1, 1, 1))
    odd, even = (0.2, 0.2, 0.25), (0.725, 0.71, 0.68)
    tex = be.texture_checker(odd, even) if record is None else be.texture_procedural(record, odd, even)
    be.rect(AXIS_XZ, -400, 400, -800, 100, 0, False, be.mat_matte(tex=tex), None)
    be.preprocess()
    return be


def export_reference_layout(root, n_lon=187, n_lat=188):
    """Writes the synthetic assets in the directory layout main.cc expects (scene/cornellbox/*.obj, scene/bunny/bunny.obj)
    for the command-line front end (jet-pbrt_amd/host/jetpbrt --assets ROOT)."""
    os.makedirs(os.path.join(root, "cornellbox"), exist_ok=True)
    os.makedirs(os.path.join(root, "bunny"), exist_ok=True)
    for name, quads in CORNELL.items():
        quads_to_obj(os.path.join(root, "cornellbox", name + ".obj"), quads)
    v, f = bunny_mesh(n_lon, n_lat)
    write_obj(os.path.join(root, "bunny", "bunny.obj"), v, f)
    return root


if __name__ == "__main__":
    import sys
    print(export_reference_layout(sys.argv[1] if len(sys.argv) > 1 else "scene"))
