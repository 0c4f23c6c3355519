"""jet-pbrt_amd -- MI355X-native path-tracing integrator behind jet-pbrt's Render() seam.

Python here is plumbing only (ctypes bindings for tests / bench / smoke): the product is
  * csrc/libjetpbrt_amd.so   hand-written HIP wavefront kernels + the C ABI of include/jetpbrt_amd.h
  * host/libjetpbrt_host.so  C++ mirror of the reference's FScene/FCamera/FFilm/FSampler/FMaterial/
                             FIntegrator::Render API, BVH builder and scene flattener.
Nothing in this package imports, links or calls anything under oracle/ (test infrastructure).
The directory name has a hyphen; import it as `jet_pbrt_amd` (shim module at the repo root).
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
HIP_LIB_PATH = os.environ.get("JETPBRT_AMD_LIB") or os.path.join(PKG_DIR, "csrc", "libjetpbrt_amd.so")   # env override: A/B of kernel builds
HOST_LIB_PATH = os.path.join(PKG_DIR, "host", "libjetpbrt_host.so")
CLI_PATH = os.path.join(PKG_DIR, "host", "jetpbrt")

JP_MAT_PARAM_STRIDE = 16
JP_SAMPLER_STOCK_MT19937, JP_SAMPLER_COUNTER, JP_SAMPLER_DEBUG = 0, 1, 2
JP_OK = 0

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class JpCamera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("front", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("res_x", C.c_float), ("res_y", C.c_float)]


class JpScene(C.Structure):
    _fields_ = [
        ("camera", JpCamera),
        ("n_triangles", C.c_int32), ("tri_p0", _fp), ("tri_p1", _fp), ("tri_p2", _fp), ("tri_n", _fp),
        ("n_rectangles", C.c_int32), ("rect_p0", _fp), ("rect_p1", _fp), ("rect_p2", _fp), ("rect_p3", _fp), ("rect_n", _fp),
        ("n_spheres", C.c_int32), ("sph_center", _fp), ("sph_radius", _fp),
        ("n_primitives", C.c_int32), ("prim_shape_type", _ip), ("prim_shape_index", _ip), ("prim_material", _ip), ("prim_light", _ip),
        ("n_materials", C.c_int32), ("mat_type", _ip), ("mat_params", _fp),
        ("n_lights", C.c_int32), ("light_type", _ip), ("light_radiance", _fp), ("light_prim", _ip), ("light_vec", _fp),
        ("world_radius", C.c_float),
        ("n_bvh_nodes", C.c_int32), ("bvh_bounds", _fp), ("bvh_left", _ip), ("bvh_right", _ip),
        ("n_bvh_prim_indices", C.c_int32), ("bvh_prim_index", _ip),
        ("bvh_reference_semantics", C.c_int32),
        ("n_disks", C.c_int32), ("disk_center", _fp), ("disk_normal", _fp), ("disk_radius", _fp),
    ]


class JpRenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("sampler_mode", C.c_int32), ("seed", C.c_uint32),
                ("band_rows", C.c_int32), ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("integrator", C.c_int32)]


class JpCounters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("closest_rays", C.c_uint64), ("closest_hits", C.c_uint64),
                ("shadow_rays", C.c_uint64), ("shadow_occluded", C.c_uint64),
                ("render_ms", C.c_double), ("extend_ms", C.c_double), ("shade_ms", C.c_double), ("shadow_ms", C.c_double),
                ("other_ms", C.c_double),
                ("extend_launches", C.c_uint64), ("shade_launches", C.c_uint64), ("shadow_launches", C.c_uint64),
                ("path_ms", C.c_double), ("path_launches", C.c_uint64), ("certified_fallback_rays", C.c_uint64)]


class JpBuildInfo(C.Structure):
    _fields_ = [("built_on_device", C.c_int32), ("traversal_mode", C.c_int32), ("bvh_nodes", C.c_int32), ("bvh_height", C.c_int32),
                ("device_build_ms", C.c_double), ("libm_sincosf", C.c_int32), ("lanes_last_render", C.c_int32),
                ("fused_last_render", C.c_int32), ("fused_region", C.c_int32), ("fused_workgroups", C.c_int32), ("q4_nodes", C.c_int32), ("libm_xbsdf", C.c_int32), ("certified_walk", C.c_int32), ("certified_nodes", C.c_int32), ("certified_eye_leaves", C.c_int32)]


JP_INTEGRATOR_PATH, JP_INTEGRATOR_WHITTED, JP_INTEGRATOR_DEBUG_NORMAL = 0, 1, 2
JP_ABI_VERSION = 7      # include/jetpbrt_amd.h; hip_lib() refuses a library built for another ABI


class JpOptions(C.Structure):
    """ABI 7: the switches of the library by value (include/jetpbrt_amd.h: JpOptions); 0 = default, tri-state switches 1 on / -1 off"""
    _fields_ = [("struct_bytes", C.c_int32), ("lanes", C.c_int32), ("lane_rows", C.c_int32), ("blocks_per_cu", C.c_int32), ("max_slots", C.c_int64),
                ("compact_regions", C.c_int32), ("fused", C.c_int32), ("fused_region", C.c_int32), ("fused_job_spp", C.c_int32), ("fused_workgroups", C.c_int32),
                ("traversal", C.c_int32), ("q4", C.c_int32), ("q4_shadow", C.c_int32), ("persist", C.c_int32), ("vote", C.c_int32), ("stack_lds_words", C.c_int32),
                ("shade_sort", C.c_int32), ("device_tree", C.c_int32), ("device_wide", C.c_int32), ("bvh_max_leaf", C.c_int32), ("ploc_radius", C.c_int32), ("ploc_max_rounds", C.c_int32),
                ("certified", C.c_int32), ("cert_slack", C.c_float), ("cert_slack_eye", C.c_float), ("cert_eye_tau", C.c_float),
                ("libm_sincosf", C.c_int32), ("libm_xbsdf", C.c_int32), ("trace_walk", C.c_int32), ("box_pad", C.c_float), ("reserved", C.c_int32 * 8)]


class JpBsdfDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("color", C.c_float * 3), ("color2", C.c_float * 3), ("eta_a", C.c_float), ("eta_b", C.c_float),
                ("distribution", C.c_int32), ("alpha_x", C.c_float), ("alpha_y", C.c_float), ("sample_visible", C.c_int32), ("fresnel", C.c_int32),
                ("fr_eta_i", C.c_float * 3), ("fr_eta_t", C.c_float * 3), ("fr_k", C.c_float * 3), ("exponent", C.c_float)]


JP_TEXTURE_SOLID, JP_TEXTURE_CHECKER, JP_TEXTURE_IMAGE = 0, 1, 2


class JpTextures(C.Structure):
    """include/jetpbrt_amd.h: JpTextures (jp_upload_scene_textured); struct_bytes = sizeof(JpTextures)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_textures", C.c_int32), ("tex_type", _ip), ("tex_color", _fp),
                ("tex_width", _ip), ("tex_height", _ip), ("tex_offset", C.POINTER(C.c_int64)),
                ("n_texel_bytes", C.c_int64), ("texels", C.POINTER(C.c_uint8)),
                ("n_materials", C.c_int32), ("mat_texture", _ip), ("n_triangles", C.c_int32), ("tri_uv", _fp)]


class JpTextureInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_textures", C.c_int32), ("n_textured_materials", C.c_int32),
                ("texel_bytes_device", C.c_int64), ("textured_last_render", C.c_int32)]


class JpDenoiseParams(C.Structure):
    """include/jetpbrt_amd.h: JpDenoiseParams (jp_denoise); struct_bytes = sizeof(JpDenoiseParams); fields left 0 take the library's defaults"""
    _fields_ = [("struct_bytes", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("demodulate", C.c_int32)]


class JpDenoiseInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulated", C.c_int32), ("guide_spp", C.c_int32), ("denoise_ms", C.c_double), ("guides_ms", C.c_double)]


JP_LIGHTS_ALL, JP_LIGHTS_POWER_ONE = 0, 1
LIGHT_SAMPLING_MODES = {None: JP_LIGHTS_ALL, "all": JP_LIGHTS_ALL, "power": JP_LIGHTS_POWER_ONE, JP_LIGHTS_ALL: JP_LIGHTS_ALL, JP_LIGHTS_POWER_ONE: JP_LIGHTS_POWER_ONE}


class JpLightSampling(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32)]


class JpLightInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32), ("n_lights", C.c_int32), ("n_selectable", C.c_int32),
                ("total_weight", C.c_double), ("picked_last_render", C.c_int32)]


JP_ESTIMATOR_NEE, JP_ESTIMATOR_MIS = 0, 1
ESTIMATOR_MODES = {None: JP_ESTIMATOR_NEE, "nee": JP_ESTIMATOR_NEE, "mis": JP_ESTIMATOR_MIS, JP_ESTIMATOR_NEE: JP_ESTIMATOR_NEE, JP_ESTIMATOR_MIS: JP_ESTIMATOR_MIS}


class JpEstimator(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32)]


class JpEstimatorInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32), ("mis_last_render", C.c_int32), ("side_bytes_device", C.c_int64)]


JP_ENV_UP_Z, JP_ENV_UP_Y = 0, 1
ENV_UP_AXES = {"z": JP_ENV_UP_Z, "y": JP_ENV_UP_Y, JP_ENV_UP_Z: JP_ENV_UP_Z, JP_ENV_UP_Y: JP_ENV_UP_Y}


class JpEnvMap(C.Structure):
    """include/jetpbrt_amd.h: JpEnvMap (jp_set_environment_map); struct_bytes = sizeof(JpEnvMap)"""
    _fields_ = [("struct_bytes", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("up_axis", C.c_int32), ("importance", C.c_int32), ("rgb", _fp)]


class JpEnvInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("up_axis", C.c_int32), ("importance", C.c_int32),
                ("n_selectable", C.c_int32), ("total_weight", C.c_double), ("mean_sum", C.c_double), ("mapped_last_render", C.c_int32),
                ("table_bytes_device", C.c_int64)]


class JpVertexNormals(C.Structure):
    """include/jetpbrt_amd.h: JpVertexNormals (jp_set_vertex_normals); struct_bytes = sizeof(JpVertexNormals)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_triangles", C.c_int32), ("tri_vn", _fp)]


class JpNormalInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_triangles", C.c_int32), ("n_smooth_triangles", C.c_int32), ("table_bytes_device", C.c_int64),
                ("smooth_last_render", C.c_int32), ("normal_ms", C.c_double)]


def vertex_normals(tri_vn):
    """A JpVertexNormals over an (n_triangles, 9) float32 array: n0 n1 n2 per triangle, nine zeros = flat (kept alive on the returned object as ._keep)"""
    import numpy as np
    a = np.ascontiguousarray(tri_vn, np.float32).reshape(-1, 9)
    v = JpVertexNormals(C.sizeof(JpVertexNormals), a.shape[0], a.ctypes.data_as(_fp))
    v._keep = a
    return v


def check_vertex_normals(tri_vn):
    """jp_check_vertex_normals: the validation of jp_set_vertex_normals (pure host code, no GPU) -> number of smooth triangles; raises JetPbrtError with its message"""
    v = tri_vn if isinstance(tri_vn, JpVertexNormals) else vertex_normals(tri_vn)
    n = C.c_int32(0)
    L = hip_lib()
    st = L.jp_check_vertex_normals(C.byref(v), C.byref(n))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return n.value


def interpolate_normals(p0, p1, p2, ng, vn9, p):
    """jp_interpolate_normals: the shading normal the device computes (include/jp_normals.h) for n points; (n, 3) arrays, vn9 (n, 9) -> (n, 3) float32.  Pure host code."""
    import numpy as np
    a = [np.ascontiguousarray(x, np.float32) for x in (p0, p1, p2, ng, vn9, p)]
    n = a[0].shape[0]
    out = np.zeros((n, 3), np.float32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    st = L.jp_interpolate_normals(n, q(a[0]), q(a[1]), q(a[2]), q(a[3]), q(a[4]), q(a[5]), q(out))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return out


class JpNormalMaps(C.Structure):
    """include/jetpbrt_amd.h: JpNormalMaps (jp_set_normal_maps); struct_bytes = sizeof(JpNormalMaps)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_maps", C.c_int32), ("map_width", _ip), ("map_height", _ip),
                ("map_offset", C.POINTER(C.c_int64)), ("n_texel_bytes", C.c_int64), ("texels", C.POINTER(C.c_uint8)),
                ("n_materials", C.c_int32), ("mat_map", _ip), ("mat_strength", _fp), ("n_triangles", C.c_int32), ("tri_uv", _fp)]


class JpNormalMapInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_maps", C.c_int32), ("n_mapped_materials", C.c_int32), ("texel_bytes_device", C.c_int64),
                ("table_bytes_device", C.c_int64), ("mapped_last_render", C.c_int32), ("normal_map_ms", C.c_double)]


def normal_maps(maps, mat_map, mat_strength=None, tri_uv=None, n_triangles=None):
    """A JpNormalMaps: maps a list of (h, w, 3) uint8 arrays (top row first), mat_map one map index per material (-1: none), mat_strength one float per
    material or None (1 for all), tri_uv an (n_triangles, 6) float32 array or None (then n_triangles gives the count).  The arrays are kept alive on the
    returned object as ._keep."""
    import numpy as np
    imgs = [np.ascontiguousarray(m, np.uint8) for m in maps]
    for m in imgs:
        if m.ndim != 3 or m.shape[2] != 3:
            raise ValueError("a normal map is an (h, w, 3) uint8 array")
    w = np.array([m.shape[1] for m in imgs], np.int32); h = np.array([m.shape[0] for m in imgs], np.int32)
    sizes = [m.size for m in imgs]
    off = np.array([sum(sizes[:i]) for i in range(len(imgs))], np.int64)
    tex = np.concatenate([m.reshape(-1) for m in imgs]) if imgs else np.zeros(0, np.uint8)
    mm = np.ascontiguousarray(mat_map, np.int32).reshape(-1)
    st = None if mat_strength is None else np.ascontiguousarray(mat_strength, np.float32).reshape(-1)
    if st is not None and st.shape[0] != mm.shape[0]:
        raise ValueError("mat_strength needs one value per material")
    uv = None if tri_uv is None else np.ascontiguousarray(tri_uv, np.float32).reshape(-1, 6)
    nt = uv.shape[0] if uv is not None else int(n_triangles or 0)
    v = JpNormalMaps(C.sizeof(JpNormalMaps), len(imgs), w.ctypes.data_as(_ip), h.ctypes.data_as(_ip), off.ctypes.data_as(C.POINTER(C.c_int64)), tex.size,
                     tex.ctypes.data_as(C.POINTER(C.c_uint8)), mm.shape[0], mm.ctypes.data_as(_ip), st.ctypes.data_as(_fp) if st is not None else None,
                     nt, uv.ctypes.data_as(_fp) if uv is not None else None)
    v._keep = (w, h, off, tex, mm, st, uv)
    return v


def _hip_status(L, st):
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))


def check_normal_maps(maps):
    """jp_check_normal_maps: the validation of jp_set_normal_maps (pure host code, no GPU) on a JpNormalMaps -> number of materials with a map; raises JetPbrtError with its message"""
    n = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_check_normal_maps(C.byref(maps), C.byref(n)))
    return n.value


def perturb_normals(nb, ng, dpdu, dpdv, uv, rgb8, strength=1.0):
    """jp_perturb_normals: the shading normal the device computes under a normal map (include/jp_normal_map.h) for n points; nb ng dpdu dpdv (n, 3), uv (n, 2),
    rgb8 an (h, w, 3) uint8 map -> (ns (n, 3) float32, perturbed (n,) int32).  Pure host code."""
    import numpy as np
    a = [np.ascontiguousarray(x, np.float32) for x in (nb, ng, dpdu, dpdv, uv)]
    img = np.ascontiguousarray(rgb8, np.uint8)
    n = a[0].shape[0]
    ns = np.zeros((n, 3), np.float32); on = np.zeros(n, np.int32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_perturb_normals(n, q(a[0]), q(a[1]), q(a[2]), q(a[3]), q(a[4]), img.shape[1], img.shape[0], q(img), float(strength), q(ns), q(on)))
    return ns, on


JP_WRAP_CLAMP, JP_WRAP_REPEAT, JP_WRAP_MIRROR = 0, 1, 2
JP_FILTER_DEFAULT, JP_FILTER_NEAREST, JP_FILTER_BILINEAR = 0, 1, 2


class JpTexSampler(C.Structure):
    """include/jetpbrt_amd.h: JpTexSampler, one texture's or one normal map's sampling record"""
    _fields_ = [("wrap_u", C.c_int32), ("wrap_v", C.c_int32), ("filter", C.c_int32), ("scale_u", C.c_float), ("scale_v", C.c_float),
                ("offset_u", C.c_float), ("offset_v", C.c_float)]


class JpTextureSampling(C.Structure):
    """include/jetpbrt_amd.h: JpTextureSampling (jp_set_texture_sampling); struct_bytes = sizeof(JpTextureSampling)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_textures", C.c_int32), ("tex", C.POINTER(JpTexSampler)), ("n_maps", C.c_int32), ("map", C.POINTER(JpTexSampler))]


class JpTexSamplingInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_active_textures", C.c_int32), ("n_active_maps", C.c_int32), ("table_bytes_device", C.c_int64),
                ("sampled_last_render", C.c_int32), ("texel_ms", C.c_double), ("normal_map_ms", C.c_double)]


def tex_sampler(wrap_u=JP_WRAP_CLAMP, wrap_v=None, filter=JP_FILTER_DEFAULT, scale=(1.0, 1.0), offset=(0.0, 0.0)):
    """A JpTexSampler; wrap_v None: wrap_u on both axes.  The defaults are the identity record."""
    return JpTexSampler(int(wrap_u), int(wrap_u if wrap_v is None else wrap_v), int(filter), float(scale[0]), float(scale[1]), float(offset[0]), float(offset[1]))


def texture_sampling(tex=None, maps=None):
    """A JpTextureSampling: tex / maps a list of JpTexSampler (None entries: the identity), one per texture / per normal map of the next upload, or None for
    none of that kind.  The arrays are kept alive on the returned object as ._keep."""
    def arr(lst):
        if lst is None:
            return 0, None
        a = (JpTexSampler * max(1, len(lst)))()
        for i, s in enumerate(lst):
            a[i] = tex_sampler() if s is None else s
        return len(lst), a
    nt, at = arr(tex); nm, am = arr(maps)
    v = JpTextureSampling(C.sizeof(JpTextureSampling), nt, at if at is None else C.cast(at, C.POINTER(JpTexSampler)), nm, am if am is None else C.cast(am, C.POINTER(JpTexSampler)))
    v._keep = (at, am)
    return v


def check_texture_sampling(sampling):
    """jp_check_texture_sampling: the validation of jp_set_texture_sampling (pure host code, no GPU) -> (n_active_textures, n_active_maps); raises JetPbrtError
    with its message"""
    a = C.c_int32(0); b = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_check_texture_sampling(C.byref(sampling), C.byref(a), C.byref(b)))
    return a.value, b.value


def texture_lookup(sampler, rgb8, uv):
    """jp_texture_lookup: the bytes the device's lookup delivers (include/jp_tex_sampling.h) for n uv pairs on the (h, w, 3) uint8 image under `sampler` (None: the
    lookup without records) -> (n, 3) uint8; the colour is (1 / 255) * byte.  Pure host code."""
    import numpy as np
    img = np.ascontiguousarray(rgb8, np.uint8)
    c = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((c.shape[0], 3), np.uint8)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_texture_lookup(None if sampler is None else C.byref(sampler), img.shape[1], img.shape[0], q(img), c.shape[0], q(c), q(out)))
    return out


def perturb_normals_sampled(sampler, nb, ng, dpdu, dpdv, uv, rgb8, strength=1.0):
    """jp_perturb_normals_sampled: perturb_normals with the map addressed through `sampler` (None: perturb_normals).  Pure host code."""
    import numpy as np
    a = [np.ascontiguousarray(x, np.float32) for x in (nb, ng, dpdu, dpdv, uv)]
    img = np.ascontiguousarray(rgb8, np.uint8)
    n = a[0].shape[0]
    ns = np.zeros((n, 3), np.float32); on = np.zeros(n, np.int32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_perturb_normals_sampled(None if sampler is None else C.byref(sampler), n, q(a[0]), q(a[1]), q(a[2]), q(a[3]), q(a[4]), img.shape[1], img.shape[0],
                                                q(img), float(strength), q(ns), q(on)))
    return ns, on


JP_MIP_OFF, JP_MIP_TRILINEAR = 0, 1


class JpTextureMipmaps(C.Structure):
    """include/jetpbrt_amd.h: JpTextureMipmaps (jp_set_texture_mipmaps); struct_bytes = sizeof(JpTextureMipmaps)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_textures", C.c_int32), ("mode", C.POINTER(C.c_int32)), ("footprint_scale", C.c_float), ("bounce_spread", C.c_float)]


class JpTextureMipmapInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_on", C.c_int32), ("n_levels", C.c_int32), ("mip_last_render", C.c_int32), ("pyramid_bytes_device", C.c_int64),
                ("cone_bytes_device", C.c_int64), ("build_ms", C.c_double), ("texel_ms", C.c_double), ("footprint_scale", C.c_float), ("bounce_spread", C.c_float),
                ("gamma0", C.c_float)]


def texture_mipmaps(modes, footprint_scale=0.0, bounce_spread=0.0):
    """A JpTextureMipmaps: modes a list of JP_MIP_OFF / JP_MIP_TRILINEAR (or booleans), one per texture of the next upload.  footprint_scale 0: 1;
    bounce_spread 0: 0.125 rad.  The array is kept alive on the returned object as ._keep."""
    a = (C.c_int32 * max(1, len(modes)))(*[int(m) for m in modes])
    v = JpTextureMipmaps(C.sizeof(JpTextureMipmaps), len(modes), C.cast(a, C.POINTER(C.c_int32)), float(footprint_scale), float(bounce_spread))
    v._keep = a
    return v


def check_texture_mipmaps(mipmaps):
    """jp_check_texture_mipmaps: the validation of jp_set_texture_mipmaps (pure host code, no GPU) -> n_on; raises JetPbrtError with its message"""
    a = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_check_texture_mipmaps(C.byref(mipmaps), C.byref(a)))
    return a.value


def build_mip_chain(rgb8):
    """jp_build_mip_chain: the pyramid of an (h, w, 3) uint8 image -> list of (h_k, w_k, 3) uint8 levels, level 0 first.  Pure host code."""
    import numpy as np
    img = np.ascontiguousarray(rgb8, np.uint8)
    h, w = img.shape[0], img.shape[1]
    lw = (C.c_int32 * 16)(); lh = (C.c_int32 * 16)(); n = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_build_mip_chain(w, h, None, None, lw, lh, C.byref(n)))
    total = sum(lw[k] * lh[k] for k in range(n.value))
    out = np.zeros(3 * total, np.uint8)
    _hip_status(L, L.jp_build_mip_chain(w, h, img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), lw, lh, C.byref(n)))
    return _split_chain(out, [(lw[k], lh[k]) for k in range(n.value)])


def _split_chain(flat, sizes):
    levels, at = [], 0
    for w, h in sizes:
        levels.append(flat[3 * at:3 * (at + w * h)].reshape(h, w, 3).copy())
        at += w * h
    return levels


def mip_level_sizes(w, h):
    """The (w_k, h_k) of every level of a w x h image's pyramid (jp_build_mip_chain without an image)."""
    lw = (C.c_int32 * 16)(); lh = (C.c_int32 * 16)(); n = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_build_mip_chain(int(w), int(h), None, None, lw, lh, C.byref(n)))
    return [(lw[k], lh[k]) for k in range(n.value)]


def mip_cone_step(gamma0, bounce_spread, flags, t, state):
    """jp_mip_cone_step: one hit for each of n independent cones; state (n, 2) float32 (width, spread) before the hit -> the state after it (a new array).  Pure host code."""
    import numpy as np
    f = np.ascontiguousarray(flags, np.int32); tt = np.ascontiguousarray(t, np.float32)
    st = np.array(state, np.float32).reshape(-1, 2).copy()
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_mip_cone_step(float(gamma0), float(bounce_spread), f.shape[0], q(f), q(tt), q(st)))
    return st


def mip_footprint(width, area, w, h, scale=(1.0, 1.0), footprint_scale=1.0):
    """jp_mip_footprint: rho in texels from the cone's width and the world area per unit uv area at the hit -> (n,) float32.  Pure host code."""
    import numpy as np
    a = np.ascontiguousarray(width, np.float32); b = np.ascontiguousarray(area, np.float32)
    out = np.zeros(a.shape[0], np.float32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_mip_footprint(a.shape[0], q(a), q(b), int(w), int(h), float(scale[0]), float(scale[1]), float(footprint_scale), q(out)))
    return out


def texture_lookup_mip(sampler, rgb8, uv, rho):
    """jp_texture_lookup_mip: texture_lookup at a footprint of rho texels per lookup, on the image's pyramid -> (n, 3) uint8.  Pure host code."""
    import numpy as np
    img = np.ascontiguousarray(rgb8, np.uint8)
    c = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    r = np.ascontiguousarray(rho, np.float32)
    out = np.zeros((c.shape[0], 3), np.uint8)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_texture_lookup_mip(None if sampler is None else C.byref(sampler), img.shape[1], img.shape[0], q(img), c.shape[0], q(c), q(r), q(out)))
    return out


JP_PROC_NONE, JP_PROC_NOISE, JP_PROC_FBM, JP_PROC_TURBULENCE, JP_PROC_MARBLE, JP_PROC_CHECKER_AA = 0, 1, 2, 3, 4, 5
JP_PROC_SPACE_WORLD, JP_PROC_SPACE_UV = 0, 1
PROC_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class JpProcedural(C.Structure):
    """include/jetpbrt_amd.h: JpProcedural (one record of jp_set_texture_procedurals)"""
    _fields_ = [("kind", C.c_int32), ("space", C.c_int32), ("m", C.c_float * 12), ("octaves", C.c_int32), ("gain", C.c_float), ("variation", C.c_float),
                ("antialias", C.c_int32)]


class JpTextureProcedurals(C.Structure):
    """include/jetpbrt_amd.h: JpTextureProcedurals (jp_set_texture_procedurals); struct_bytes = sizeof(JpTextureProcedurals)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_textures", C.c_int32), ("rec", C.POINTER(JpProcedural))]


class JpProceduralInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_procedural", C.c_int32), ("n_antialiased", C.c_int32), ("procedural_last_render", C.c_int32),
                ("table_bytes_device", C.c_int64)]


def procedural(kind, space=JP_PROC_SPACE_WORLD, m=PROC_IDENTITY, octaves=0, gain=0.0, variation=0.0, antialias=0):
    """A JpProcedural: kind JP_PROC_*, m the row-major 3 x 4 map into texture space; octaves 0: 6, gain 0: 0.5, variation 0: 1, antialias 0 / 1: on, -1: off"""
    return JpProcedural(int(kind), int(space), (C.c_float * 12)(*[float(x) for x in m]), int(octaves), float(gain), float(variation), int(antialias))


def texture_procedurals(records):
    """A JpTextureProcedurals: one JpProcedural (or None: JP_PROC_NONE) per texture of the next upload.  The array is kept alive on the returned object as ._keep."""
    a = (JpProcedural * max(1, len(records)))()
    for i, r in enumerate(records):
        if r is not None:
            a[i] = r
    v = JpTextureProcedurals(C.sizeof(JpTextureProcedurals), len(records), C.cast(a, C.POINTER(JpProcedural)))
    v._keep = a
    return v


def check_texture_procedurals(procedurals, textures=None):
    """jp_check_texture_procedurals: the validation of jp_set_texture_procedurals and, with a JpTextures, of the upload (pure host code, no GPU)
    -> (n_procedural, n_antialiased); raises JetPbrtError with its message"""
    a = C.c_int32(0); b = C.c_int32(0)
    L = hip_lib()
    _hip_status(L, L.jp_check_texture_procedurals(C.byref(procedurals), None if textures is None else C.byref(textures), C.byref(a), C.byref(b)))
    return a.value, b.value


def procedural_lookup(record, c_even, c_odd, p, uv, width, texture=0):
    """jp_procedural_lookup: the side words (n,) uint32 and blend parameters t (n,) float32 of one record at n points: p (n, 3), uv (n, 2), width (n,).
    Pure host code."""
    import numpy as np
    pp = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n = pp.shape[0]
    u = np.ascontiguousarray(np.broadcast_to(np.asarray(uv, np.float32), (n, 2)))
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(width, np.float32), (n,)))
    ce = (C.c_float * 3)(*[float(x) for x in c_even]); co = (C.c_float * 3)(*[float(x) for x in c_odd])
    word = np.zeros(n, np.uint32); t = np.zeros(n, np.float32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_procedural_lookup(C.byref(record), ce, co, int(texture), n, q(pp), q(u), q(w), q(word), q(t)))
    return word, t


def triangle_tangents(p0, p1, p2, uv6):
    """jp_triangle_tangents: dpdu, dpdv of n triangles from their corners (n, 3) and uvs (n, 6) -> (dpdu (n, 3), dpdv (n, 3), ok (n,) int32).  Pure host code."""
    import numpy as np
    a = [np.ascontiguousarray(x, np.float32) for x in (p0, p1, p2, uv6)]
    n = a[0].shape[0]
    du = np.zeros((n, 3), np.float32); dv = np.zeros((n, 3), np.float32); ok = np.zeros(n, np.int32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_triangle_tangents(n, q(a[0]), q(a[1]), q(a[2]), q(a[3]), q(du), q(dv), q(ok)))
    return du, dv, ok


class JpLens(C.Structure):
    """include/jetpbrt_amd.h: JpLens (jp_set_lens); struct_bytes = sizeof(JpLens)"""
    _fields_ = [("struct_bytes", C.c_int32), ("radius", C.c_float), ("focus_distance", C.c_float), ("blades", C.c_int32), ("rotation_deg", C.c_float)]


class JpLensInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("radius", C.c_float), ("focus_distance", C.c_float), ("blades", C.c_int32), ("rotation_deg", C.c_float),
                ("lens_last_render", C.c_int32)]


JP_LENS_MAX_BLADES = 16


class JpLensPlan(C.Structure):
    """include/jp_lens.h: JpLensPlan, what the kernels receive by value (jp_lens_plan)"""
    _fields_ = [("radius", C.c_float), ("focus", C.c_float), ("n_verts", C.c_int32), ("ex", C.c_float * 3), ("ey", C.c_float * 3),
                ("v", (C.c_float * 2) * (JP_LENS_MAX_BLADES + 1))]


def lens(radius, focus_distance=1.0, blades=0, rotation_deg=0.0):
    """A JpLens (or pass one through)"""
    return radius if isinstance(radius, JpLens) else JpLens(C.sizeof(JpLens), radius, focus_distance, blades, rotation_deg)


def _lens_ptr(l):
    return None if l is None else C.byref(l)


def check_lens(l):
    """jp_check_lens: the validation of jp_set_lens (pure host code, no GPU); raises JetPbrtError with its message.  l: a JpLens or None"""
    L = hip_lib()
    st = L.jp_check_lens(_lens_ptr(l))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))


def lens_plan(camera, l):
    """jp_lens_plan: the JpLensPlan of lens `l` (a JpLens or None) on a JpCamera (pure host code, no GPU) -> JpLensPlan, or None for the pinhole"""
    L = hip_lib()
    n = C.c_int64(0)
    plan = JpLensPlan()
    st = L.jp_lens_plan(C.byref(camera), _lens_ptr(l), C.byref(plan), C.sizeof(plan), C.byref(n))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    if n.value == 0:
        return None
    if n.value != C.sizeof(plan):
        raise JetPbrtError("jp_lens_plan: the library's JpLensPlan has %d bytes, this binding's %d" % (n.value, C.sizeof(plan)))
    return plan


def lens_rays(camera, l, fxfy, u=None):
    """jp_lens_rays: the camera rays the device forms (include/jp_lens.h) for film positions fxfy (n, 2) and lens draws u (n, 2) through lens `l`
    (a JpLens, or None for the pinhole) -> (origin (n, 3), dir (n, 3)) float32.  Pure host code."""
    import numpy as np
    f = np.ascontiguousarray(fxfy, np.float32).reshape(-1, 2)
    n = f.shape[0]
    uu = None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 2)
    if uu is not None and uu.shape[0] != n:
        raise JetPbrtError("lens_rays: fxfy and u differ in length")
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    q = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    st = L.jp_lens_rays(C.byref(camera), _lens_ptr(l), n, q(f), q(uu), q(o), q(d))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return o, d


JP_PROJ_PERSPECTIVE, JP_PROJ_ORTHOGRAPHIC, JP_PROJ_EQUIRECT, JP_PROJ_FISHEYE = 0, 1, 2, 3
JP_FIT_DIAGONAL, JP_FIT_WIDTH, JP_FIT_HEIGHT = 0, 1, 2
PROJECTIONS = {"perspective": JP_PROJ_PERSPECTIVE, "ortho": JP_PROJ_ORTHOGRAPHIC, "orthographic": JP_PROJ_ORTHOGRAPHIC, "equirect": JP_PROJ_EQUIRECT,
               "fisheye": JP_PROJ_FISHEYE}
FITS = {"diagonal": JP_FIT_DIAGONAL, "width": JP_FIT_WIDTH, "height": JP_FIT_HEIGHT}


class JpProjection(C.Structure):
    """include/jetpbrt_amd.h: JpProjection (jp_set_projection); struct_bytes = sizeof(JpProjection)"""
    _fields_ = [("struct_bytes", C.c_int32), ("kind", C.c_int32), ("ortho_scale", C.c_float), ("fov_deg", C.c_float), ("fit", C.c_int32)]


class JpProjectionInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("kind", C.c_int32), ("ortho_scale", C.c_float), ("fov_deg", C.c_float), ("fit", C.c_int32),
                ("projected_last_render", C.c_int32), ("gamma0_last_render", C.c_float)]


class JpProjectionPlan(C.Structure):
    """include/jp_projection.h: JpProjectionPlan, what the kernels receive by value (jp_projection_plan)"""
    _fields_ = [("kind", C.c_int32), ("scale", C.c_float), ("half_fov", C.c_float), ("R", C.c_float), ("gamma0", C.c_float),
                ("ex", C.c_float * 3), ("ey", C.c_float * 3), ("ez", C.c_float * 3)]


def projection(kind, ortho_scale=0.0, fov_deg=0.0, fit=JP_FIT_DIAGONAL):
    """A JpProjection (or pass one through).  kind: JP_PROJ_* or "ortho" / "equirect" / "fisheye" / "perspective"; fit: JP_FIT_* or "diagonal" / "width" / "height";
    ortho_scale 0: 1, fov_deg 0: 180"""
    if isinstance(kind, JpProjection):
        return kind
    k = PROJECTIONS[kind] if isinstance(kind, str) else kind
    f = FITS[fit] if isinstance(fit, str) else fit
    return JpProjection(C.sizeof(JpProjection), k, ortho_scale, fov_deg, f)


def check_projection(p):
    """jp_check_projection: the validation of jp_set_projection (pure host code, no GPU); raises JetPbrtError with its message.  p: a JpProjection or None"""
    L = hip_lib()
    st = L.jp_check_projection(_lens_ptr(p))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))


def projection_plan(camera, p):
    """jp_projection_plan: the JpProjectionPlan of projection `p` (a JpProjection or None) on a JpCamera (pure host code, no GPU) -> JpProjectionPlan, or None
    for the pinhole"""
    L = hip_lib()
    n = C.c_int64(0)
    plan = JpProjectionPlan()
    st = L.jp_projection_plan(C.byref(camera), _lens_ptr(p), C.byref(plan), C.sizeof(plan), C.byref(n))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    if n.value == 0:
        return None
    if n.value != C.sizeof(plan):
        raise JetPbrtError("jp_projection_plan: the library's JpProjectionPlan has %d bytes, this binding's %d" % (n.value, C.sizeof(plan)))
    return plan


def projection_rays(camera, p, fxfy):
    """jp_projection_rays: the camera rays the device forms (include/jp_projection.h) for film positions fxfy (n, 2) under projection `p` (a JpProjection, or
    None for the pinhole) -> (origin (n, 3), dir (n, 3)) float32.  Pure host code."""
    import numpy as np
    f = np.ascontiguousarray(fxfy, np.float32).reshape(-1, 2)
    n = f.shape[0]
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    st = L.jp_projection_rays(C.byref(camera), _lens_ptr(p), n, q(f), q(o), q(d))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return o, d


JP_FILM_BINS = 256
JP_CURVE_CLAMP, JP_CURVE_REINHARD, JP_CURVE_ACES, JP_CURVE_HABLE = 0, 1, 2, 3
JP_EXPOSURE_MANUAL, JP_EXPOSURE_AUTO = 0, 1
CURVES = {"clamp": JP_CURVE_CLAMP, "reinhard": JP_CURVE_REINHARD, "aces": JP_CURVE_ACES, "hable": JP_CURVE_HABLE}


class JpFilm(C.Structure):
    """include/jetpbrt_amd.h: JpFilm (jp_set_film); struct_bytes = sizeof(JpFilm)"""
    _fields_ = [("struct_bytes", C.c_int32), ("hdr", C.c_int32), ("sample_clamp", C.c_float)]


class JpFilmInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("hdr", C.c_int32), ("sample_clamp", C.c_float), ("hdr_last_render", C.c_int32)]


class JpToneMap(C.Structure):
    """include/jetpbrt_amd.h: JpToneMap (jp_set_tonemap, jp_tonemap); struct_bytes = sizeof(JpToneMap); key, white and the percentiles left 0 take the defaults"""
    _fields_ = [("struct_bytes", C.c_int32), ("curve", C.c_int32), ("exposure_mode", C.c_int32), ("ev", C.c_float), ("key", C.c_float), ("white", C.c_float),
                ("pct_low", C.c_float), ("pct_high", C.c_float)]


class JpToneMapInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("curve", C.c_int32), ("exposure_mode", C.c_int32), ("scale_last", C.c_float), ("mapped_last_render", C.c_int32),
                ("histogram_ms", C.c_double), ("tonemap_ms", C.c_double)]


class JpVarianceInfo(C.Structure):
    """include/jetpbrt_amd.h: JpVarianceInfo (jp_get_variance_info)"""
    _fields_ = [("struct_bytes", C.c_int32), ("variance_last_render", C.c_int32), ("moment_bytes_device", C.c_int64), ("iterations", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("demodulated", C.c_int32), ("denoise_ms", C.c_double)]


class JpAdaptive(C.Structure):
    """include/jetpbrt_amd.h: JpAdaptive (jp_render_adaptive); struct_bytes = sizeof(JpAdaptive); max_spp 0: JpRenderParams.spp, floor 0: 1e-3"""
    _fields_ = [("struct_bytes", C.c_int32), ("min_spp", C.c_int32), ("step_spp", C.c_int32), ("max_spp", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float),
                ("dilate", C.c_int32)]


class JpAdaptiveInfo(C.Structure):
    """include/jetpbrt_amd.h: JpAdaptiveInfo (jp_get_adaptive_info)"""
    _fields_ = [("struct_bytes", C.c_int32), ("adaptive_last_render", C.c_int32), ("passes", C.c_int32), ("min_spp", C.c_int32), ("step_spp", C.c_int32),
                ("max_spp", C.c_int32), ("dilate", C.c_int32), ("threshold", C.c_float), ("samples_traced", C.c_int64), ("state_bytes_device", C.c_int64),
                ("active_after", C.c_int32 * 16), ("select_ms", C.c_double), ("resolve_ms", C.c_double)]


def adaptive(threshold, min_spp=8, step_spp=8, max_spp=0, floor=0.0, dilate=1):
    """A JpAdaptive (or pass one through)"""
    return threshold if isinstance(threshold, JpAdaptive) else JpAdaptive(C.sizeof(JpAdaptive), min_spp, step_spp, max_spp, threshold, floor, int(dilate))


def film(hdr=1, sample_clamp=0.0):
    """A JpFilm (or pass one through)"""
    return hdr if isinstance(hdr, JpFilm) else JpFilm(C.sizeof(JpFilm), int(hdr), sample_clamp)


def tonemap(curve=JP_CURVE_CLAMP, exposure="manual", ev=0.0, key=0.0, white=0.0, pct_low=0.0, pct_high=0.0):
    """A JpToneMap (or pass one through): curve a JP_CURVE_* or its name, exposure "manual" / "auto" or a JP_EXPOSURE_*"""
    if isinstance(curve, JpToneMap):
        return curve
    mode = {"manual": JP_EXPOSURE_MANUAL, "auto": JP_EXPOSURE_AUTO}.get(exposure, exposure)
    return JpToneMap(C.sizeof(JpToneMap), CURVES.get(curve, curve), mode, ev, key, white, pct_low, pct_high)


def _ptr(s):
    return None if s is None else C.byref(s)


def check_film(f):
    """jp_check_film: the validation of jp_set_film (pure host code, no GPU); raises JetPbrtError with its message.  f: a JpFilm or None"""
    L = hip_lib()
    _hip_status(L, L.jp_check_film(_ptr(f)))


def check_tonemap(t):
    """jp_check_tonemap: the validation of jp_set_tonemap (pure host code, no GPU); raises JetPbrtError with its message.  t: a JpToneMap or None"""
    L = hip_lib()
    _hip_status(L, L.jp_check_tonemap(_ptr(t)))


def film_samples(f, rgb):
    """jp_film_samples: the per-sample clamp of JpFilm `f` (or None) on (n, 3) float32 radiances -> (n, 3) float32.  Pure host code, the function the device runs."""
    import numpy as np
    a = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    out = np.zeros_like(a)
    L = hip_lib()
    _hip_status(L, L.jp_film_samples(_ptr(f), a.shape[0], a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def variance_samples(f, samples, want_mean=False):
    """jp_variance_samples: the per-pixel variance of the mean luminance of (spp, n, 3) float32 samples under JpFilm `f` (or None) -> (n,) float32
    [, the running mean (n,)].  Pure host code, the function the device runs."""
    import numpy as np
    a = np.ascontiguousarray(samples, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise JetPbrtError("variance_samples: samples must be (spp, n, 3)")
    spp, n = a.shape[:2]
    var = np.zeros(n, np.float32); mean = np.zeros(n, np.float32)
    L = hip_lib()
    _hip_status(L, L.jp_variance_samples(_ptr(f), spp, n, a.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), mean.ctypes.data_as(C.c_void_p)))
    return (var, mean) if want_mean else var


def check_adaptive(a):
    """jp_check_adaptive: the validation of jp_render_adaptive (pure host code, no GPU); raises JetPbrtError with its message.  a: a JpAdaptive or None"""
    L = hip_lib()
    _hip_status(L, L.jp_check_adaptive(_ptr(a)))


def _adaptive_planes(fn, a, f, samples, height, width):
    import numpy as np
    s = np.ascontiguousarray(samples, np.float32)
    if s.ndim != 3 or s.shape[2] != 3 or s.shape[1] != height * width:
        raise JetPbrtError("adaptive samples must be (max_spp, height * width, 3)")
    if a.max_spp != 0 and a.max_spp != s.shape[0]:
        raise JetPbrtError("adaptive samples: %d samples per pixel given, max_spp is %d" % (s.shape[0], a.max_spp))
    if a.max_spp == 0:
        a = JpAdaptive(a.struct_bytes, a.min_spp, a.step_spp, s.shape[0], a.threshold, a.floor, a.dilate)
    film_ = np.zeros((height, width, 3), np.float32); counts = np.zeros((height, width), np.int32); var = np.zeros((height, width), np.float32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)
    fn(_ptr(f), C.byref(a), width, height, q(s), q(film_), q(counts), q(var))
    return film_, counts, var


def adaptive_samples(f, a, samples, height, width):
    """jp_adaptive_samples: the whole adaptive loop of JpAdaptive `a` under JpFilm `f` (or None) on (max_spp, height * width, 3) float32 samples ->
    (film (H, W, 3) float32, counts (H, W) int32, variance (H, W) float32).  Pure host code, the functions the device runs."""
    L = hip_lib()
    return _adaptive_planes(lambda *args: _hip_status(L, L.jp_adaptive_samples(*args)), a, f, samples, height, width)


def exposure_from_histogram(t, hist):
    """jp_exposure_from_histogram: the exposure scale of JpToneMap `t` for a histogram of JP_FILM_BINS + 1 counts (None with manual exposure).  Pure host code."""
    import numpy as np
    h = None if hist is None else np.ascontiguousarray(hist, np.uint32)
    if h is not None and h.size != JP_FILM_BINS + 1:
        raise JetPbrtError("exposure_from_histogram: the histogram has JP_FILM_BINS + 1 counts")
    s = C.c_float(0)
    L = hip_lib()
    _hip_status(L, L.jp_exposure_from_histogram(C.byref(t), None if h is None else h.ctypes.data_as(C.c_void_p), C.byref(s)))
    return s.value


def tonemap_host(t, scale, values, want_bytes=True, want_floats=True):
    """jp_tonemap_host: the display transform of JpToneMap `t` under `scale` on an array of float32 values -> (uint8 array or None, float32 array or None) of its
    shape.  Pure host code, the function the device runs."""
    import numpy as np
    a = np.ascontiguousarray(values, np.float32)
    b = np.zeros(a.shape, np.uint8) if want_bytes else None
    f = np.zeros(a.shape, np.float32) if want_floats else None
    q = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    _hip_status(L, L.jp_tonemap_host(C.byref(t), C.c_float(scale), a.size, q(a), q(b), q(f)))
    return b, f


def env_map(rgb, up_axis=JP_ENV_UP_Z, importance=0):
    """A JpEnvMap over an (H, W, 3) float32 array, top row first (kept alive on the returned object as ._keep)"""
    import numpy as np
    a = np.ascontiguousarray(rgb, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise JetPbrtError("an environment map is an (H, W, 3) array")
    m = JpEnvMap(C.sizeof(JpEnvMap), a.shape[1], a.shape[0], ENV_UP_AXES[up_axis], importance, a.ctypes.data_as(_fp))
    m._keep = a
    return m


def build_environment_table(rgb, tint=(1.0, 1.0, 1.0), up_axis=JP_ENV_UP_Z, importance=0):
    """jp_build_environment_table: the tables the upload makes of an (H, W, 3) map and a tint (pure host code, no GPU) ->
    dict(weight float64 (H*W), q float32, alias int32, texel float32 (H*W, 4), row_cos float32 (H, 2), total, mean_sum).
    rgb may also be a ready JpEnvMap (refusal tests)."""
    import numpy as np
    m = rgb if isinstance(rgb, JpEnvMap) else env_map(rgb, up_axis, importance)
    n = max(0, m.width) * max(0, m.height) if 0 < m.width <= 4096 and 0 < m.height <= 4096 else 0
    out = dict(weight=np.zeros(n, np.float64), q=np.zeros(n, np.float32), alias=np.zeros(n, np.int32), texel=np.zeros((n, 4), np.float32),
               row_cos=np.zeros((m.height if n else 0, 2), np.float32))
    t = np.ascontiguousarray(tint, np.float32)
    tot, mean = C.c_double(0.0), C.c_double(0.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    st = L.jp_build_environment_table(C.byref(m), p(t), p(out["weight"]), p(out["q"]), p(out["alias"]), p(out["texel"]), p(out["row_cos"]), C.byref(tot), C.byref(mean))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    out["total"], out["mean_sum"] = tot.value, mean.value
    return out


UPLOAD_TABLES = ("nodes", "prims", "meta", "mats", "mat_type", "lights", "shade_tab", "wide", "q4", "refbox", "flat")


class JpUploadTable(C.Structure):
    _fields_ = [("bytes", C.c_int64), ("fnv1a", C.c_uint64)]


class JpUploadInfo(C.Structure):
    """include/jetpbrt_amd.h: JpUploadInfo (jp_describe_upload); table[i] belongs to UPLOAD_TABLES[i]"""
    _fields_ = [("struct_bytes", C.c_int32), ("trav_mode", C.c_int32), ("stack_depth", C.c_int32), ("stack_depth_q4", C.c_int32),
                ("lds_bytes", C.c_int64), ("lds_bytes_shadow", C.c_int64), ("shade_lds_bytes", C.c_int64),
                ("scene_in_lds", C.c_int32), ("tables_in_lds", C.c_int32), ("shade_prims_in_lds", C.c_int32), ("stage_nee", C.c_int32), ("n_planes", C.c_int32),
                ("persist", C.c_int32), ("vote", C.c_int32), ("shade_sort", C.c_int32), ("use_q4", C.c_int32), ("q4_shadow", C.c_int32), ("cert", C.c_int32),
                ("class_mask", C.c_int32), ("shape_mask", C.c_int32), ("light_mask", C.c_int32), ("light_shape_mask", C.c_int32),
                ("has_null_material", C.c_int32), ("stack_lds_words", C.c_int32),
                ("n_nodes", C.c_int32), ("n_prims", C.c_int32), ("n_flat", C.c_int32), ("n_wide", C.c_int32), ("n_q4", C.c_int32),
                ("bvh_nodes", C.c_int32), ("bvh_height", C.c_int32), ("wide_height", C.c_int32), ("q4_height", C.c_int32), ("cert_eye_leaves", C.c_int32), ("n_env", C.c_int32),
                ("cert_pad", C.c_float), ("cert_pad_eye", C.c_float), ("env_sum", C.c_float * 3),
                ("table", JpUploadTable * len(UPLOAD_TABLES))]


def describe_upload(scene, options=None, light_mode=JP_LIGHTS_ALL):
    """jp_describe_upload: what jp_upload_scene would decide for `scene` (a JpScene or a pointer to one) and the digests of the tables it would
    copy to the device (pure host code, no GPU).  options: a JpOptions, or None for the defaults without the environment -> JpUploadInfo"""
    L = hip_lib()
    info = JpUploadInfo()
    info.struct_bytes = C.sizeof(JpUploadInfo)
    if options is not None:
        options.struct_bytes = C.sizeof(JpOptions)
    st = L.jp_describe_upload(None if options is None else C.byref(options), LIGHT_SAMPLING_MODES[light_mode], scene if isinstance(scene, C._Pointer) else C.byref(scene), C.byref(info))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return info


class JpTreeInfo(C.Structure):
    """include/jetpbrt_amd.h: JpTreeInfo (jp_get_tree_info)"""
    _fields_ = [("struct_bytes", C.c_int32), ("n_prims", C.c_int32), ("n_nodes", C.c_int32), ("bvh_height", C.c_int32), ("n_wide", C.c_int32), ("wide_height", C.c_int32),
                ("n_q4", C.c_int32), ("q4_height", C.c_int32), ("n_flat", C.c_int32)]


def _table_index(which):
    return UPLOAD_TABLES.index(which) if isinstance(which, str) else int(which)


def _read_table(call):
    """the size query, then the copy, of jp_copy_upload_table / jp_read_scene_table -> the table's bytes as a uint8 array (empty: no such table)"""
    import numpy as np
    n = C.c_int64(0)
    st = call(None, 0, C.byref(n))
    if st == JP_OK:
        out = np.zeros(n.value, np.uint8)
        if n.value:
            st = call(out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, hip_lib().jp_last_error().decode()))
    return out


def copy_upload_table(scene, which, options=None, light_mode=JP_LIGHTS_ALL):
    """jp_copy_upload_table: the bytes jp_upload_scene would copy to the device for table `which` (a name of UPLOAD_TABLES or its index) of `scene`
    (a JpScene or a pointer to one): what JpUploadInfo.table[which] counts and hashes (pure host code, no GPU) -> uint8 array"""
    L = hip_lib()
    if options is not None:
        options.struct_bytes = C.sizeof(JpOptions)
    o = None if options is None else C.byref(options)
    sp = scene if isinstance(scene, C._Pointer) else C.byref(scene)
    return _read_table(lambda out, cap, n: L.jp_copy_upload_table(o, LIGHT_SAMPLING_MODES[light_mode], sp, _table_index(which), out, cap, n))


def build_light_table(weights):
    """jp_build_light_table: the alias table of the upload for `weights` (pure host code, no GPU) -> (q float32, alias int32, pmf float32)"""
    import numpy as np
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    n = w.shape[0]
    q = np.zeros(n, np.float32); alias = np.zeros(n, np.int32); pmf = np.zeros(n, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = hip_lib()
    st = L.jp_build_light_table(n, p(w), p(q), p(alias), p(pmf))
    if st != JP_OK:
        raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, L.jp_last_error().decode()))
    return q, alias, pmf


def denoise_params(width, height, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, demodulate=0):
    return JpDenoiseParams(C.sizeof(JpDenoiseParams), width, height, iterations, sigma_color, sigma_normal, sigma_depth, demodulate)


def textures(tex_type, tex_color, mat_texture, n_triangles=0, tri_uv=None, images=()):
    """A JpTextures over numpy arrays (kept alive on the returned object as ._keep).  tex_type / tex_color (n, 6) / mat_texture as in the
    header; images: {texture index: (H, W, 3) uint8 array} -- their texels are packed one after another."""
    import numpy as np
    n = len(tex_type)
    tt = np.ascontiguousarray(tex_type, np.int32); tc = np.ascontiguousarray(np.asarray(tex_color, np.float32).reshape(n, 6))
    w = np.zeros(n, np.int32); h = np.zeros(n, np.int32); off = np.zeros(n, np.int64)
    chunks, at = [], 0
    for k, img in dict(images).items():
        img = np.ascontiguousarray(img, np.uint8)
        h[k], w[k], off[k] = img.shape[0], img.shape[1], at
        chunks.append(img.reshape(-1)); at += img.size
    tx = np.ascontiguousarray(np.concatenate(chunks) if chunks else np.zeros(1, np.uint8))
    mt = np.ascontiguousarray(mat_texture, np.int32)
    t = JpTextures()
    t.struct_bytes = C.sizeof(JpTextures); t.n_textures = n
    t.tex_type = tt.ctypes.data_as(_ip); t.tex_color = tc.ctypes.data_as(_fp); t.tex_width = w.ctypes.data_as(_ip); t.tex_height = h.ctypes.data_as(_ip)
    t.tex_offset = off.ctypes.data_as(C.POINTER(C.c_int64)); t.n_texel_bytes = at; t.texels = tx.ctypes.data_as(C.POINTER(C.c_uint8))
    t.n_materials = len(mt); t.mat_texture = mt.ctypes.data_as(_ip); t.n_triangles = n_triangles
    uv = None
    if tri_uv is not None:
        uv = np.ascontiguousarray(tri_uv, np.float32); t.tri_uv = uv.ctypes.data_as(_fp)
    t._keep = (tt, tc, w, h, off, tx, mt, uv)
    return t


JP_BSDF_LAMBERT, JP_BSDF_MIRROR, JP_BSDF_FRESNEL_SPECULAR, JP_BSDF_MICROFACET_REFLECTION, JP_BSDF_MICROFACET_TRANSMISSION, JP_BSDF_PHONG = range(6)
JP_DIST_TROWBRIDGE_REITZ, JP_DIST_BECKMANN = 0, 1
JP_FRESNEL_CONDUCTOR, JP_FRESNEL_DIELECTRIC, JP_FRESNEL_NOOP = 0, 1, 2


def bsdf_desc(kind, color=(1, 1, 1), color2=(1, 1, 1), eta_a=1.0, eta_b=1.5, distribution=0, alpha=(0.2, 0.2), sample_visible=True, fresnel=0,
              fr_eta_i=(1, 1, 1), fr_eta_t=(1.5, 1.5, 1.5), fr_k=(0, 0, 0), exponent=10.0):
    d = JpBsdfDesc()
    d.kind = kind; d.color[:] = color; d.color2[:] = color2; d.eta_a = eta_a; d.eta_b = eta_b; d.distribution = distribution
    d.alpha_x, d.alpha_y = alpha; d.sample_visible = 1 if sample_visible else 0; d.fresnel = fresnel
    d.fr_eta_i[:] = fr_eta_i; d.fr_eta_t[:] = fr_eta_t; d.fr_k[:] = fr_k; d.exponent = exponent
    return d


def render_params(width, height, spp, max_depth=5, seed=1234, sampler_mode=JP_SAMPLER_COUNTER,
                  band_rows=20, shard_index=0, shard_count=1, integrator=JP_INTEGRATOR_PATH):
    return JpRenderParams(width, height, spp, max_depth, sampler_mode, seed, band_rows, shard_index, shard_count, integrator)


class JetPbrtError(RuntimeError):
    pass


_host = None
_hip = None


def host_lib():
    """libjetpbrt_host.so (C++ host mirror + flattener).  Raises if it has not been built."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise JetPbrtError("host library missing: %s (run __graft_entry__.build())" % HOST_LIB_PATH)
        L = C.CDLL(HOST_LIB_PATH)
        L.jp_host_scene_new.restype = C.c_void_p
        L.jp_host_scene_new.argtypes = [C.c_char_p]
        L.jp_host_scene_free.argtypes = [C.c_void_p]
        L.jp_host_last_error.restype = C.c_char_p
        L.jp_host_last_error.argtypes = [C.c_void_p]
        L.jp_host_scene_camera.argtypes = [C.c_void_p, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float]
        L.jp_host_scene_envlight.argtypes = [C.c_void_p, _fp]
        L.jp_host_scene_pointlight.argtypes = [C.c_void_p, _fp, _fp]
        L.jp_host_scene_dirlight.argtypes = [C.c_void_p, _fp, _fp]
        L.jp_host_mat_matte.argtypes = [C.c_void_p, _fp]
        L.jp_host_mat_mirror.argtypes = [C.c_void_p, _fp]
        L.jp_host_mat_glass.argtypes = [C.c_void_p, C.c_float, _fp, _fp]
        L.jp_host_mat_plastic.argtypes = [C.c_void_p, _fp, _fp, C.c_float, C.c_int]
        L.jp_host_mat_metal.argtypes = [C.c_void_p, _fp, _fp, C.c_float, C.c_float, C.c_int]
        L.jp_host_scene_mesh.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, _fp, C.c_float, C.c_int, _fp]
        L.jp_host_scene_rect.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _fp]
        L.jp_host_scene_sphere.argtypes = [C.c_void_p, _fp, C.c_float, C.c_int, _fp]
        L.jp_host_scene_disk.argtypes = [C.c_void_p, _fp, _fp, C.c_float, C.c_int, _fp]
        L.jp_host_scene_preprocess.argtypes = [C.c_void_p]
        L.jp_host_scene_set_device_build.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_scene_set_reference_tree.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_num_primitives.argtypes = [C.c_void_p]
        L.jp_host_num_lights.argtypes = [C.c_void_p]
        L.jp_host_flatten.restype = C.POINTER(JpScene)
        L.jp_host_flatten.argtypes = [C.c_void_p]
        L.jp_host_render.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.POINTER(JpCounters)]
        L.jp_host_render_other.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p]
        L.jp_host_save_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.jp_host_render_ldr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        L.jp_host_gamma_encode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.jp_host_bsdf_class.argtypes = [C.c_int, _fp, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, _fp, _fp, _fp, _fp, _fp]
        L.jp_host_texture_solid.argtypes = [C.c_void_p, _fp]
        L.jp_host_texture_checker.argtypes = [C.c_void_p, _fp, _fp]
        L.jp_host_texture_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.jp_host_texture_image_file.argtypes = [C.c_void_p, C.c_char_p]
        L.jp_host_mat_matte_tex.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_mat_mirror_tex.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_mat_plastic_tex.argtypes = [C.c_void_p, C.c_int, _fp, C.c_float, C.c_int]
        L.jp_host_mat_set_texture.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.jp_host_flatten_textures.restype = C.POINTER(JpTextures)
        L.jp_host_flatten_textures.argtypes = [C.c_void_p]
        L.jp_host_render_sampler.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.jp_host_render_denoised.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.jp_host_render_variance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint] + [C.c_int] * 5 + [C.c_void_p] * 5
        L.jp_host_render_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_float] + [C.c_int] * 6 + [C.c_void_p] * 3
        L.jp_host_render_film.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                          C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_char_p, C.c_int]
        L.jp_host_scene_set_light_sampling.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_scene_set_estimator.argtypes = [C.c_void_p, C.c_int]
        L.jp_host_scene_set_lens.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float]
        L.jp_host_scene_set_projection.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]
        L.jp_host_last_focus.restype = C.c_float
        L.jp_host_last_focus.argtypes = [C.c_void_p]
        L.jp_host_scene_envmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.jp_host_scene_envmap_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.jp_host_scene_mesh_smooth.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, _fp, C.c_float, C.c_int, _fp, C.c_int, C.c_float]
        L.jp_host_flatten_normals.restype = C.POINTER(JpVertexNormals)
        L.jp_host_flatten_normals.argtypes = [C.c_void_p]
        L.jp_host_normal_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.jp_host_normal_map_file.argtypes = [C.c_void_p, C.c_char_p]
        L.jp_host_normal_map_from_height.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
        L.jp_host_normal_map_read.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        L.jp_host_mat_set_normal_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
        L.jp_host_flatten_normal_maps.restype = C.POINTER(JpNormalMaps)
        L.jp_host_flatten_normal_maps.argtypes = [C.c_void_p]
        L.jp_host_texture_set_sampling.argtypes = [C.c_void_p, C.c_int, C.POINTER(JpTexSampler)]
        L.jp_host_normal_map_set_sampling.argtypes = [C.c_void_p, C.c_int, C.POINTER(JpTexSampler)]
        L.jp_host_scene_set_texture_sampling_default.argtypes = [C.c_void_p, C.POINTER(JpTexSampler)]
        L.jp_host_flatten_texture_sampling.restype = C.POINTER(JpTextureSampling)
        L.jp_host_flatten_texture_sampling.argtypes = [C.c_void_p]
        L.jp_host_texture_set_mipmaps.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.jp_host_scene_set_texture_mipmap_default.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.jp_host_flatten_texture_mipmaps.restype = C.POINTER(JpTextureMipmaps)
        L.jp_host_flatten_texture_procedurals.restype = C.POINTER(JpTextureProcedurals)
        L.jp_host_flatten_texture_procedurals.argtypes = [C.c_void_p]
        L.jp_host_texture_procedural.argtypes = [C.c_void_p, C.POINTER(JpProcedural), C.c_void_p, C.c_void_p]
        L.jp_host_normal_map_from_procedural.argtypes = [C.c_void_p, C.POINTER(JpProcedural), C.c_int, C.c_int, C.c_float]
        L.jp_host_flatten_texture_mipmaps.argtypes = [C.c_void_p]
        L.jp_host_flatten_envmap.restype = C.POINTER(JpEnvMap)
        L.jp_host_flatten_envmap.argtypes = [C.c_void_p]
        _host = L
    return _host


def hip_lib():
    """libjetpbrt_amd.so (HIP kernels + C ABI).  Raises loudly if missing: there is no CPU fallback."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise JetPbrtError("HIP library missing: %s (run __graft_entry__.build()); the product has no CPU fallback" % HIP_LIB_PATH)
        L = C.CDLL(HIP_LIB_PATH)
        if L.jp_abi_version() != JP_ABI_VERSION:                 # (a stale or foreign build would be handed structs of the wrong size)
            raise JetPbrtError("%s implements ABI %d, this binding ABI %d: rebuild with __graft_entry__.build()" % (HIP_LIB_PATH, L.jp_abi_version(), JP_ABI_VERSION))
        L.jp_last_error.restype = C.c_char_p
        L.jp_set_options.argtypes = [C.c_void_p, C.POINTER(JpOptions)]
        L.jp_get_options.argtypes = [C.c_void_p, C.POINTER(JpOptions)]
        L.jp_create_context.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.jp_destroy_context.argtypes = [C.c_void_p]
        L.jp_upload_scene.argtypes = [C.c_void_p, C.POINTER(JpScene)]
        L.jp_render.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_void_p]
        L.jp_render_device.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_void_p, C.c_int]
        L.jp_synchronize.argtypes = [C.c_void_p]
        L.jp_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.jp_get_counters.argtypes = [C.c_void_p, C.POINTER(JpCounters)]
        L.jp_get_build_info.argtypes = [C.c_void_p, C.POINTER(JpBuildInfo)]
        L.jp_trace.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
        L.jp_occluded.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(C.c_int32)]
        L.jp_render_rgb8.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_void_p, C.c_void_p]
        L.jp_gamma_thresholds.argtypes = [C.c_void_p]
        L.jp_bsdf.argtypes = [C.c_void_p, C.POINTER(JpBsdfDesc), C.c_int32] + [C.c_void_p] * 10
        L.jp_upload_scene_textured.argtypes = [C.c_void_p, C.POINTER(JpScene), C.POINTER(JpTextures)]
        L.jp_get_texture_info.argtypes = [C.c_void_p, C.POINTER(JpTextureInfo)]
        L.jp_surface.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        L.jp_render_guides.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_int32] + [C.c_void_p] * 3
        L.jp_render_guides_device.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_int32] + [C.c_void_p] * 3 + [C.c_int]
        L.jp_denoise.argtypes = [C.c_void_p, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 5
        L.jp_denoise_device.argtypes = [C.c_void_p, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 5 + [C.c_int]
        L.jp_get_denoise_info.argtypes = [C.c_void_p, C.POINTER(JpDenoiseInfo)]
        L.jp_set_light_sampling.argtypes = [C.c_void_p, C.POINTER(JpLightSampling)]
        L.jp_get_light_info.argtypes = [C.c_void_p, C.POINTER(JpLightInfo)]
        L.jp_get_light_table.argtypes = [C.c_void_p] * 4
        L.jp_light_pick.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        L.jp_build_light_table.argtypes = [C.c_int32] + [C.c_void_p] * 4
        L.jp_device_bytes_in_use.restype = C.c_longlong
        L.jp_set_estimator.argtypes = [C.c_void_p, C.POINTER(JpEstimator)]
        L.jp_get_estimator_info.argtypes = [C.c_void_p, C.POINTER(JpEstimatorInfo)]
        L.jp_light_pdf.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.jp_set_environment_map.argtypes = [C.c_void_p, C.POINTER(JpEnvMap)]
        L.jp_get_env_info.argtypes = [C.c_void_p, C.POINTER(JpEnvInfo)]
        L.jp_env_lookup.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 3
        L.jp_env_sample.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
        L.jp_build_environment_table.argtypes = [C.POINTER(JpEnvMap)] + [C.c_void_p] * 6 + [C.POINTER(C.c_double)] * 2
        L.jp_describe_upload.argtypes = [C.POINTER(JpOptions), C.c_int32, C.POINTER(JpScene), C.POINTER(JpUploadInfo)]
        L.jp_copy_upload_table.argtypes = [C.POINTER(JpOptions), C.c_int32, C.POINTER(JpScene), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.jp_read_scene_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.jp_get_tree_info.argtypes = [C.c_void_p, C.POINTER(JpTreeInfo)]
        L.jp_set_vertex_normals.argtypes = [C.c_void_p, C.POINTER(JpVertexNormals)]
        L.jp_get_normal_info.argtypes = [C.c_void_p, C.POINTER(JpNormalInfo)]
        L.jp_shading_normal.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        L.jp_interpolate_normals.argtypes = [C.c_int32] + [C.c_void_p] * 7
        L.jp_check_vertex_normals.argtypes = [C.POINTER(JpVertexNormals), C.POINTER(C.c_int32)]
        L.jp_set_normal_maps.argtypes = [C.c_void_p, C.POINTER(JpNormalMaps)]
        L.jp_check_normal_maps.argtypes = [C.POINTER(JpNormalMaps), C.POINTER(C.c_int32)]
        L.jp_get_normal_map_info.argtypes = [C.c_void_p, C.POINTER(JpNormalMapInfo)]
        L.jp_perturb_normals.argtypes = [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.jp_set_texture_sampling.argtypes = [C.c_void_p, C.POINTER(JpTextureSampling)]
        L.jp_check_texture_sampling.argtypes = [C.POINTER(JpTextureSampling), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.jp_get_texture_sampling_info.argtypes = [C.c_void_p, C.POINTER(JpTexSamplingInfo)]
        L.jp_texture_lookup.argtypes = [C.POINTER(JpTexSampler), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.jp_perturb_normals_sampled.argtypes = [C.POINTER(JpTexSampler), C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.jp_triangle_tangents.argtypes = [C.c_int32] + [C.c_void_p] * 7
        L.jp_set_texture_mipmaps.argtypes = [C.c_void_p, C.POINTER(JpTextureMipmaps)]
        L.jp_check_texture_mipmaps.argtypes = [C.POINTER(JpTextureMipmaps), C.POINTER(C.c_int32)]
        L.jp_get_texture_mipmap_info.argtypes = [C.c_void_p, C.POINTER(JpTextureMipmapInfo)]
        L.jp_read_mip_chain.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.jp_build_mip_chain.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.jp_mip_cone_step.argtypes = [C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jp_mip_footprint.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.jp_texture_lookup_mip.argtypes = [C.POINTER(JpTexSampler), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jp_mip_probe.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
        L.jp_set_texture_procedurals.argtypes = [C.c_void_p, C.POINTER(JpTextureProcedurals)]
        L.jp_check_texture_procedurals.argtypes = [C.POINTER(JpTextureProcedurals), C.POINTER(JpTextures), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.jp_get_procedural_info.argtypes = [C.c_void_p, C.POINTER(JpProceduralInfo)]
        L.jp_procedural_lookup.argtypes = [C.POINTER(JpProcedural), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_int32] + [C.c_void_p] * 5
        L.jp_procedural_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
        L.jp_set_lens.argtypes = [C.c_void_p, C.POINTER(JpLens)]
        L.jp_get_lens_info.argtypes = [C.c_void_p, C.POINTER(JpLensInfo)]
        L.jp_check_lens.argtypes = [C.POINTER(JpLens)]
        L.jp_lens_plan.argtypes = [C.POINTER(JpCamera), C.POINTER(JpLens), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.jp_lens_rays.argtypes = [C.POINTER(JpCamera), C.POINTER(JpLens), C.c_int32] + [C.c_void_p] * 4
        L.jp_camera_rays.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_int32] + [C.c_void_p] * 6
        L.jp_set_projection.argtypes = [C.c_void_p, C.POINTER(JpProjection)]
        L.jp_get_projection_info.argtypes = [C.c_void_p, C.POINTER(JpProjectionInfo)]
        L.jp_check_projection.argtypes = [C.POINTER(JpProjection)]
        L.jp_projection_plan.argtypes = [C.POINTER(JpCamera), C.POINTER(JpProjection), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.jp_projection_rays.argtypes = [C.POINTER(JpCamera), C.POINTER(JpProjection), C.c_int32] + [C.c_void_p] * 3
        L.jp_focus_distance.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.jp_render_denoised.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_int32, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 5
        L.jp_set_film.argtypes = [C.c_void_p, C.POINTER(JpFilm)]
        L.jp_check_film.argtypes = [C.POINTER(JpFilm)]
        L.jp_get_film_info.argtypes = [C.c_void_p, C.POINTER(JpFilmInfo)]
        L.jp_film_samples.argtypes = [C.POINTER(JpFilm), C.c_int32, C.c_void_p, C.c_void_p]
        L.jp_film_histogram.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.jp_film_histogram_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
        L.jp_set_tonemap.argtypes = [C.c_void_p, C.POINTER(JpToneMap)]
        L.jp_check_tonemap.argtypes = [C.POINTER(JpToneMap)]
        L.jp_exposure_from_histogram.argtypes = [C.POINTER(JpToneMap), C.c_void_p, C.POINTER(C.c_float)]
        L.jp_tonemap.argtypes = [C.c_void_p, C.POINTER(JpToneMap), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.jp_tonemap_device.argtypes = [C.c_void_p, C.POINTER(JpToneMap), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int]
        L.jp_tonemap_host.argtypes = [C.POINTER(JpToneMap), C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jp_get_tonemap_info.argtypes = [C.c_void_p, C.POINTER(JpToneMapInfo)]
        L.jp_render_variance.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_void_p, C.c_void_p]
        L.jp_render_variance_device.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_void_p, C.c_void_p, C.c_int]
        L.jp_variance_samples.argtypes = [C.POINTER(JpFilm), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jp_variance_probe.argtypes = [C.c_void_p, C.POINTER(JpFilm), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
        L.jp_denoise_variance.argtypes = [C.c_void_p, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 7
        L.jp_denoise_variance_device.argtypes = [C.c_void_p, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 7 + [C.c_int]
        L.jp_render_denoised_variance.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.c_int32, C.POINTER(JpDenoiseParams)] + [C.c_void_p] * 6
        L.jp_get_variance_info.argtypes = [C.c_void_p, C.POINTER(JpVarianceInfo)]
        L.jp_check_adaptive.argtypes = [C.POINTER(JpAdaptive)]
        L.jp_render_adaptive.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.POINTER(JpAdaptive), C.c_void_p, C.c_void_p, C.c_void_p]
        L.jp_render_adaptive_device.argtypes = [C.c_void_p, C.POINTER(JpRenderParams), C.POINTER(JpAdaptive), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.jp_adaptive_samples.argtypes = [C.POINTER(JpFilm), C.POINTER(JpAdaptive), C.c_int32, C.c_int32] + [C.c_void_p] * 4
        L.jp_adaptive_probe.argtypes = [C.c_void_p, C.POINTER(JpFilm), C.POINTER(JpAdaptive), C.c_int32, C.c_int32] + [C.c_void_p] * 4
        L.jp_get_adaptive_info.argtypes = [C.c_void_p, C.POINTER(JpAdaptiveInfo)]
        _hip = L
    return _hip


def device_bytes_in_use():
    """Bytes of device memory the library holds in this process, over all contexts (jp_device_bytes_in_use)."""
    return int(hip_lib().jp_device_bytes_in_use())


class Context:
    """Thin RAII wrapper over JpContext for harness code."""

    def __init__(self, device_id=0):
        self.lib = hip_lib()
        self.h = C.c_void_p()
        self._check(self.lib.jp_create_context(device_id, C.byref(self.h)))

    def _check(self, st):
        if st != JP_OK:
            raise JetPbrtError("jetpbrt_amd status %d: %s" % (st, self.lib.jp_last_error().decode()))

    def get_options(self):
        o = JpOptions()
        self._check(self.lib.jp_get_options(self.h, C.byref(o)))
        return o

    def set_options(self, **kw):
        """jp_set_options: the options in force with the given fields changed (e.g. lanes=1, persist=-1); no arguments: back to the initial value.
        Traversal fields apply to the next upload, schedule fields to the next render."""
        if not kw:
            self._check(self.lib.jp_set_options(self.h, None))
            return
        o = self.get_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise JetPbrtError("JpOptions has no field %r" % k)
            setattr(o, k, v)
        o.struct_bytes = C.sizeof(JpOptions)
        self._check(self.lib.jp_set_options(self.h, C.byref(o)))

    def upload(self, scene_ptr, textures=None):
        """jp_upload_scene, or jp_upload_scene_textured when `textures` (a JpTextures or a pointer to one) is given"""
        if textures is None:
            self._check(self.lib.jp_upload_scene(self.h, scene_ptr))
        else:
            self._check(self.lib.jp_upload_scene_textured(self.h, scene_ptr, textures if isinstance(textures, C._Pointer) else C.byref(textures)))

    def texture_info(self):
        i = JpTextureInfo()
        i.struct_bytes = C.sizeof(JpTextureInfo)
        self._check(self.lib.jp_get_texture_info(self.h, C.byref(i)))
        return i

    def surface(self, origin, direction, tmin, tmax):
        """jp_surface: closest hit, the shape's uv and the colour of the textured slot -> (prim (n,), uv (n, 2), albedo (n, 3))"""
        import numpy as np
        n = origin.shape[0]
        o = np.ascontiguousarray(origin, np.float32); d = np.ascontiguousarray(direction, np.float32)
        t0 = np.ascontiguousarray(tmin, np.float32); t1 = np.ascontiguousarray(tmax, np.float32)
        prim = np.zeros(n, np.int32); uv = np.zeros((n, 2), np.float32); alb = np.zeros((n, 3), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_surface(self.h, n, p(o), p(d), p(t0), p(t1), p(prim), p(uv), p(alb)))
        return prim, uv, alb

    def render(self, params):
        import numpy as np
        film = np.zeros((params.height, params.width, 3), np.float32)
        self._check(self.lib.jp_render(self.h, C.byref(params), film.ctypes.data_as(C.c_void_p)))
        return film

    def render_rgb8(self, params, with_film=False):
        """jp_render_rgb8: the film as 8-bit gamma-encoded RGB (H, W, 3) uint8 [, and the fp32 film]"""
        import numpy as np
        rgb8 = np.zeros((params.height, params.width, 3), np.uint8)
        film = np.zeros((params.height, params.width, 3), np.float32) if with_film else None
        self._check(self.lib.jp_render_rgb8(self.h, C.byref(params), rgb8.ctypes.data_as(C.c_void_p), film.ctypes.data_as(C.c_void_p) if with_film else None))
        return (rgb8, film) if with_film else rgb8

    def render_device(self, params, device_ptr, sync=False):
        self._check(self.lib.jp_render_device(self.h, C.byref(params), C.c_void_p(device_ptr), 1 if sync else 0))

    def render_guides(self, params, guide_spp=8):
        """jp_render_guides: the first-hit feature buffers of the frame -> (albedo (H, W, 3), normal (H, W, 3), depth (H, W))"""
        import numpy as np
        alb = np.zeros((params.height, params.width, 3), np.float32); nrm = np.zeros((params.height, params.width, 3), np.float32)
        dep = np.zeros((params.height, params.width), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_render_guides(self.h, C.byref(params), guide_spp, p(alb), p(nrm), p(dep)))
        return alb, nrm, dep

    def render_guides_device(self, params, guide_spp, albedo_ptr, normal_ptr, depth_ptr, sync=False):
        """jp_render_guides_device: device pointers (any may be 0 / None), as render_device takes its film"""
        self._check(self.lib.jp_render_guides_device(self.h, C.byref(params), guide_spp, C.c_void_p(albedo_ptr or None), C.c_void_p(normal_ptr or None),
                                                     C.c_void_p(depth_ptr or None), 1 if sync else 0))

    def denoise(self, film, albedo, normal, depth, **kw):
        """jp_denoise: the edge-avoiding a-trous filter on a (H, W, 3) film with its guides -> the denoised (H, W, 3) film.
        kw: iterations, sigma_color, sigma_normal, sigma_depth, demodulate (JpDenoiseParams; 0 = the library's default)"""
        import numpy as np
        h, w = film.shape[:2]
        a = [None if x is None else np.ascontiguousarray(x, np.float32) for x in (film, albedo, normal, depth)]
        out = np.zeros((h, w, 3), np.float32)
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        dp = denoise_params(w, h, **kw)
        self._check(self.lib.jp_denoise(self.h, C.byref(dp), p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(out)))
        return out

    def denoise_device(self, width, height, film_ptr, albedo_ptr, normal_ptr, depth_ptr, out_ptr, sync=False, **kw):
        """jp_denoise_device: device pointers in the layouts jp_render_device / jp_render_guides_device write"""
        dp = denoise_params(width, height, **kw)
        self._check(self.lib.jp_denoise_device(self.h, C.byref(dp), C.c_void_p(film_ptr or None), C.c_void_p(albedo_ptr or None), C.c_void_p(normal_ptr or None),
                                               C.c_void_p(depth_ptr or None), C.c_void_p(out_ptr or None), 1 if sync else 0))

    def denoise_info(self):
        i = JpDenoiseInfo()
        i.struct_bytes = C.sizeof(JpDenoiseInfo)
        self._check(self.lib.jp_get_denoise_info(self.h, C.byref(i)))
        return i

    def set_light_sampling(self, mode):
        """jp_set_light_sampling for the next upload: None / "all" / JP_LIGHTS_ALL, or "power" / JP_LIGHTS_POWER_ONE (one light per bounce by power)"""
        if mode not in LIGHT_SAMPLING_MODES:
            raise JetPbrtError("unknown light sampling mode %r" % (mode,))
        if mode is None:
            self._check(self.lib.jp_set_light_sampling(self.h, None))
            return
        ls = JpLightSampling(C.sizeof(JpLightSampling), LIGHT_SAMPLING_MODES[mode])
        self._check(self.lib.jp_set_light_sampling(self.h, C.byref(ls)))

    def light_info(self):
        i = JpLightInfo()
        i.struct_bytes = C.sizeof(JpLightInfo)
        self._check(self.lib.jp_get_light_info(self.h, C.byref(i)))
        return i

    def light_table(self):
        """jp_get_light_table: the alias table on the device -> (q float32, alias int32, pmf float32), n_lights entries each"""
        import numpy as np
        n = self.light_info().n_lights
        q = np.zeros(n, np.float32); alias = np.zeros(n, np.int32); pmf = np.zeros(n, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_get_light_table(self.h, p(q), p(alias), p(pmf)))
        return q, alias, pmf

    def light_pick(self, u0, u1):
        """jp_light_pick: the device's selection for pairs of draws -> (index int32, pmf float32)"""
        import numpy as np
        a = np.ascontiguousarray(u0, np.float32).reshape(-1); b = np.ascontiguousarray(u1, np.float32).reshape(-1)
        n = a.shape[0]
        idx = np.zeros(n, np.int32); pmf = np.zeros(n, np.float32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_light_pick(self.h, n, p(a), p(b), p(idx), p(pmf)))
        return idx, pmf

    def set_estimator(self, mode):
        """jp_set_estimator for the next render: None / "nee" / JP_ESTIMATOR_NEE, or "mis" / JP_ESTIMATOR_MIS (needs a scene uploaded with "power" light sampling)"""
        if mode not in ESTIMATOR_MODES:
            raise JetPbrtError("unknown estimator %r" % (mode,))
        if mode is None:
            self._check(self.lib.jp_set_estimator(self.h, None))
            return
        e = JpEstimator(C.sizeof(JpEstimator), ESTIMATOR_MODES[mode])
        self._check(self.lib.jp_set_estimator(self.h, C.byref(e)))

    def estimator_info(self):
        i = JpEstimatorInfo()
        i.struct_bytes = C.sizeof(JpEstimatorInfo)
        self._check(self.lib.jp_get_estimator_info(self.h, C.byref(i)))
        return i

    def light_pdf(self, origin, direction, tmin, tmax):
        """jp_light_pdf: the light a ray reaches and the light strategy's solid-angle pdf at its origin -> (light int32 (n,), pdf float32 (n,))"""
        import numpy as np
        o = np.ascontiguousarray(origin, np.float32).reshape(-1, 3); d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = o.shape[0]
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,))); t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        light = np.zeros(n, np.int32); pdf = np.zeros(n, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_light_pdf(self.h, n, p(o), p(d), p(t0), p(t1), p(light), p(pdf)))
        return light, pdf

    def set_environment_map(self, rgb, up_axis=JP_ENV_UP_Z, importance=0):
        """jp_set_environment_map for the next upload: an (H, W, 3) float32 array top row first, a JpEnvMap, or None for no map.
        up_axis: "z" / JP_ENV_UP_Z (map space = world space) or "y" / JP_ENV_UP_Y; importance -1: sample by solid angle alone"""
        if rgb is None:
            self._check(self.lib.jp_set_environment_map(self.h, None))
            return
        m = rgb if isinstance(rgb, JpEnvMap) else env_map(rgb, up_axis, importance)
        self._check(self.lib.jp_set_environment_map(self.h, C.byref(m)))

    def env_info(self):
        i = JpEnvInfo()
        i.struct_bytes = C.sizeof(JpEnvInfo)
        self._check(self.lib.jp_get_env_info(self.h, C.byref(i)))
        return i

    def env_lookup(self, direction):
        """jp_env_lookup: the texel a world-space direction sees -> (texel index int32 (n,), tinted rgb float32 (n, 3))"""
        import numpy as np
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = d.shape[0]
        idx = np.zeros(n, np.int32); rgb = np.zeros((n, 3), np.float32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_env_lookup(self.h, n, p(d), p(idx), p(rgb)))
        return idx, rgb

    def env_sample(self, u):
        """jp_env_sample: the device's next-event sample of the map for (n, 5) draws a0 a1 a2 b0 b1 ->
        (texel index int32 (n,), wi float32 (n, 3), Li float32 (n, 3), pdf float32 (n,))"""
        import numpy as np
        a = np.ascontiguousarray(u, np.float32).reshape(-1, 5)
        n = a.shape[0]
        idx = np.zeros(n, np.int32); wi = np.zeros((n, 3), np.float32); Li = np.zeros((n, 3), np.float32); pdf = np.zeros(n, np.float32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_env_sample(self.h, n, p(a), p(idx), p(wi), p(Li), p(pdf)))
        return idx, wi, Li, pdf

    def set_lens(self, radius=None, focus_distance=1.0, blades=0, rotation_deg=0.0):
        """jp_set_lens for the next render / guides: a radius (with focus_distance, blades 0 = disk or 3 .. 16, rotation_deg), a JpLens, or None for the pinhole"""
        if radius is None:
            self._check(self.lib.jp_set_lens(self.h, None))
            return
        l = lens(radius, focus_distance, blades, rotation_deg)
        self._check(self.lib.jp_set_lens(self.h, C.byref(l)))

    def set_film(self, hdr=None, sample_clamp=0.0):
        """jp_set_film for the next render / denoise: hdr 0 / 1 (with sample_clamp, 0 = off), a JpFilm, or None for the reference's film"""
        if hdr is None:
            self._check(self.lib.jp_set_film(self.h, None))
            return
        f = film(hdr, sample_clamp)
        self._check(self.lib.jp_set_film(self.h, C.byref(f)))

    def film_info(self):
        i = JpFilmInfo()
        i.struct_bytes = C.sizeof(JpFilmInfo)
        self._check(self.lib.jp_get_film_info(self.h, C.byref(i)))
        return i

    def set_tonemap(self, curve=None, **kw):
        """jp_set_tonemap for the next render_rgb8 / render_denoised: a curve (with exposure, ev, key, white, pct_low, pct_high), a JpToneMap, or None for none"""
        if curve is None:
            self._check(self.lib.jp_set_tonemap(self.h, None))
            return
        t = tonemap(curve, **kw)
        self._check(self.lib.jp_set_tonemap(self.h, C.byref(t)))

    def tonemap_info(self):
        i = JpToneMapInfo()
        i.struct_bytes = C.sizeof(JpToneMapInfo)
        self._check(self.lib.jp_get_tonemap_info(self.h, C.byref(i)))
        return i

    def film_histogram(self, film_rgb):
        """jp_film_histogram: the luminance histogram of an (H, W, 3) film -> JP_FILM_BINS + 1 uint32 counts (the last one: the excluded pixels)"""
        import numpy as np
        a = np.ascontiguousarray(film_rgb, np.float32)
        h, w = a.shape[:2]
        hist = np.zeros(JP_FILM_BINS + 1, np.uint32)
        self._check(self.lib.jp_film_histogram(self.h, w, h, a.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p)))
        return hist

    def film_histogram_device(self, width, height, film_ptr, hist_ptr, sync=False):
        """jp_film_histogram_device: device pointers (a tightly packed rgb film, JP_FILM_BINS + 1 dwords)"""
        self._check(self.lib.jp_film_histogram_device(self.h, width, height, C.c_void_p(film_ptr or None), C.c_void_p(hist_ptr or None), 1 if sync else 0))

    def tonemap(self, film_rgb, t=None, want_bytes=True, want_floats=True):
        """jp_tonemap: the display transform of JpToneMap `t` (None: the one in force) on an (H, W, 3) film -> (rgb8 (H, W, 3) uint8 or None,
        rgb (H, W, 3) float32 or None, the exposure scale used)"""
        import numpy as np
        a = np.ascontiguousarray(film_rgb, np.float32)
        h, w = a.shape[:2]
        b = np.zeros((h, w, 3), np.uint8) if want_bytes else None
        f = np.zeros((h, w, 3), np.float32) if want_floats else None
        q = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        s = C.c_float(0)
        self._check(self.lib.jp_tonemap(self.h, _ptr(t), w, h, q(a), q(b), q(f), C.byref(s)))
        return b, f, s.value

    def tonemap_device(self, width, height, film_ptr, rgb8_ptr, rgb_ptr, t=None, sync=False):
        """jp_tonemap_device: device pointers (either output may be 0 / None) -> the exposure scale used"""
        s = C.c_float(0)
        self._check(self.lib.jp_tonemap_device(self.h, _ptr(t), width, height, C.c_void_p(film_ptr or None), C.c_void_p(rgb8_ptr or None), C.c_void_p(rgb_ptr or None),
                                               C.byref(s), 1 if sync else 0))
        return s.value

    def render_denoised(self, params, guide_spp=8, denoise=True, want_bytes=True, **kw):
        """jp_render_denoised: render, guides, the filter (denoise False: guides only) and the bytes of render_rgb8 in one call ->
        (film (H, W, 3), rgb8 (H, W, 3) or None, albedo, normal, depth).  kw: the fields of denoise_params"""
        import numpy as np
        h, w = params.height, params.width
        f = np.zeros((h, w, 3), np.float32); b = np.zeros((h, w, 3), np.uint8) if want_bytes else None
        alb = np.zeros((h, w, 3), np.float32); nrm = np.zeros((h, w, 3), np.float32); dep = np.zeros((h, w), np.float32)
        q = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        dp = denoise_params(w, h, **kw) if denoise else None
        self._check(self.lib.jp_render_denoised(self.h, C.byref(params), guide_spp, _ptr(dp), q(f), q(b), q(alb), q(nrm), q(dep)))
        return f, b, alb, nrm, dep

    def render_variance(self, params, want_film=True):
        """jp_render_variance: the film of render() and the per-pixel variance of its mean luminance -> (film (H, W, 3) or None, variance (H, W))"""
        import numpy as np
        film = np.zeros((params.height, params.width, 3), np.float32) if want_film else None
        var = np.zeros((params.height, params.width), np.float32)
        self._check(self.lib.jp_render_variance(self.h, C.byref(params), film.ctypes.data_as(C.c_void_p) if want_film else None, var.ctypes.data_as(C.c_void_p)))
        return film, var

    def render_variance_device(self, params, film_ptr, variance_ptr, sync=False):
        """jp_render_variance_device: device pointers, as render_device takes its film"""
        self._check(self.lib.jp_render_variance_device(self.h, C.byref(params), C.c_void_p(film_ptr or None), C.c_void_p(variance_ptr or None), 1 if sync else 0))

    def variance_probe(self, samples, batch_spp, f=None):
        """jp_variance_probe: the device twin of variance_samples on (spp, n, 3) float32 samples, in batches of batch_spp -> (n,) float32"""
        import numpy as np
        a = np.ascontiguousarray(samples, np.float32)
        spp, n = a.shape[:2]
        var = np.zeros(n, np.float32)
        self._check(self.lib.jp_variance_probe(self.h, _ptr(f), spp, batch_spp, n, a.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)))
        return var

    def denoise_variance(self, film, albedo, normal, depth, variance, want_variance=True, **kw):
        """jp_denoise_variance: the variance-guided a-trous filter on a (H, W, 3) film with its guides and its (H, W) variance plane ->
        (the denoised (H, W, 3) film, the filtered variance (H, W) or None).  kw: the fields of denoise_params (0 = the library's default)"""
        import numpy as np
        h, w = film.shape[:2]
        a = [None if x is None else np.ascontiguousarray(x, np.float32) for x in (film, albedo, normal, depth, variance)]
        out = np.zeros((h, w, 3), np.float32); vout = np.zeros((h, w), np.float32) if want_variance else None
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        dp = denoise_params(w, h, **kw)
        self._check(self.lib.jp_denoise_variance(self.h, C.byref(dp), p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(out), p(vout)))
        return out, vout

    def denoise_variance_device(self, width, height, film_ptr, albedo_ptr, normal_ptr, depth_ptr, variance_ptr, out_ptr, variance_out_ptr=None, sync=False, **kw):
        """jp_denoise_variance_device: device pointers in the layouts the *_device renders write"""
        dp = denoise_params(width, height, **kw)
        v = lambda x: C.c_void_p(x or None)
        self._check(self.lib.jp_denoise_variance_device(self.h, C.byref(dp), v(film_ptr), v(albedo_ptr), v(normal_ptr), v(depth_ptr), v(variance_ptr), v(out_ptr),
                                                        v(variance_out_ptr), 1 if sync else 0))

    def render_denoised_variance(self, params, guide_spp=8, denoise=True, want_bytes=True, **kw):
        """jp_render_denoised_variance: the variance render, guides, the variance-guided filter (denoise False: guides only) and the bytes of render_rgb8 in
        one call -> (film (H, W, 3), rgb8 (H, W, 3) or None, albedo, normal, depth, variance (H, W)).  kw: the fields of denoise_params"""
        import numpy as np
        h, w = params.height, params.width
        f = np.zeros((h, w, 3), np.float32); b = np.zeros((h, w, 3), np.uint8) if want_bytes else None
        alb = np.zeros((h, w, 3), np.float32); nrm = np.zeros((h, w, 3), np.float32); dep = np.zeros((h, w), np.float32); var = np.zeros((h, w), np.float32)
        q = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        dp = denoise_params(w, h, **kw) if denoise else None
        self._check(self.lib.jp_render_denoised_variance(self.h, C.byref(params), guide_spp, _ptr(dp), q(f), q(b), q(alb), q(nrm), q(dep), q(var)))
        return f, b, alb, nrm, dep, var

    def render_adaptive(self, params, a):
        """jp_render_adaptive: a render that stops each pixel by JpAdaptive `a` -> (film (H, W, 3) float32, counts (H, W) int32, variance (H, W) float32)"""
        import numpy as np
        h, w = params.height, params.width
        film_ = np.zeros((h, w, 3), np.float32); counts = np.zeros((h, w), np.int32); var = np.zeros((h, w), np.float32)
        q = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_render_adaptive(self.h, C.byref(params), _ptr(a), q(film_), q(counts), q(var)))
        return film_, counts, var

    def render_adaptive_device(self, params, a, film_ptr, counts_ptr, variance_ptr, sync=True):
        """jp_render_adaptive_device: device pointers (any two may be 0 / None), as render_device takes its film"""
        v = lambda x: C.c_void_p(x or None)
        self._check(self.lib.jp_render_adaptive_device(self.h, C.byref(params), _ptr(a), v(film_ptr), v(counts_ptr), v(variance_ptr), 1 if sync else 0))

    def adaptive_probe(self, a, samples, height, width, f=None):
        """jp_adaptive_probe: the device twin of adaptive_samples (k_resolve_list, k_adapt_select, k_adapt_finish on caller-supplied samples; no scene needed)"""
        return _adaptive_planes(lambda *args: self._check(self.lib.jp_adaptive_probe(self.h, *args)), a, f, samples, height, width)

    def adaptive_info(self):
        i = JpAdaptiveInfo()
        i.struct_bytes = C.sizeof(JpAdaptiveInfo)
        self._check(self.lib.jp_get_adaptive_info(self.h, C.byref(i)))
        return i

    def variance_info(self):
        i = JpVarianceInfo()
        i.struct_bytes = C.sizeof(JpVarianceInfo)
        self._check(self.lib.jp_get_variance_info(self.h, C.byref(i)))
        return i

    def set_projection(self, kind=None, ortho_scale=0.0, fov_deg=0.0, fit=JP_FIT_DIAGONAL):
        """jp_set_projection for the next render / guides / camera_rays: a kind (JP_PROJ_* or its name, with ortho_scale, fov_deg, fit), a JpProjection, or None
        for the pinhole"""
        if kind is None:
            self._check(self.lib.jp_set_projection(self.h, None))
            return
        p = projection(kind, ortho_scale, fov_deg, fit)
        self._check(self.lib.jp_set_projection(self.h, C.byref(p)))

    def projection_info(self):
        i = JpProjectionInfo()
        i.struct_bytes = C.sizeof(JpProjectionInfo)
        self._check(self.lib.jp_get_projection_info(self.h, C.byref(i)))
        return i

    def lens_info(self):
        i = JpLensInfo()
        i.struct_bytes = C.sizeof(JpLensInfo)
        self._check(self.lib.jp_get_lens_info(self.h, C.byref(i)))
        return i

    def camera_rays(self, params, x, y, s):
        """jp_camera_rays: what k_raygen forms for sample s[i] of pixel (x[i], y[i]) under params' seed / sampler_mode and the lens in force ->
        (origin (n, 3) float32, dir (n, 3) float32, dim_next (n,) int32)"""
        import numpy as np
        xs = np.ascontiguousarray(x, np.int32).reshape(-1); ys = np.ascontiguousarray(y, np.int32).reshape(-1); ss = np.ascontiguousarray(s, np.int32).reshape(-1)
        n = xs.shape[0]
        if ys.shape[0] != n or ss.shape[0] != n:
            raise JetPbrtError("camera_rays: x, y and s differ in length")
        o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32); k = np.zeros(n, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_camera_rays(self.h, C.byref(params), n, p(xs), p(ys), p(ss), p(o), p(d), p(k)))
        return o, d, k

    def focus_distance(self, fx, fy):
        """jp_focus_distance: the focus_distance that puts what the pinhole ray through film position (fx, fy) hits on the plane of focus; 0.0 on a miss"""
        f = C.c_float(0.0)
        self._check(self.lib.jp_focus_distance(self.h, fx, fy, C.byref(f)))
        return f.value

    def set_vertex_normals(self, tri_vn):
        """jp_set_vertex_normals for the next upload: an (n_triangles, 9) float32 array (nine zeros: a flat triangle), a JpVertexNormals, or None for none"""
        if tri_vn is None:
            self._check(self.lib.jp_set_vertex_normals(self.h, None))
            return
        v = tri_vn if isinstance(tri_vn, JpVertexNormals) else vertex_normals(tri_vn)
        self._check(self.lib.jp_set_vertex_normals(self.h, C.byref(v)))

    def normal_info(self):
        i = JpNormalInfo()
        i.struct_bytes = C.sizeof(JpNormalInfo)
        self._check(self.lib.jp_get_normal_info(self.h, C.byref(i)))
        return i

    def set_normal_maps(self, maps):
        """jp_set_normal_maps for the next upload: a JpNormalMaps (normal_maps(...) builds one), or None for none"""
        self._check(self.lib.jp_set_normal_maps(self.h, None if maps is None else C.byref(maps)))

    def normal_map_info(self):
        i = JpNormalMapInfo()
        i.struct_bytes = C.sizeof(JpNormalMapInfo)
        self._check(self.lib.jp_get_normal_map_info(self.h, C.byref(i)))
        return i

    def set_texture_sampling(self, sampling):
        """jp_set_texture_sampling for the next upload: a JpTextureSampling (texture_sampling(...) builds one), or None for none"""
        self._check(self.lib.jp_set_texture_sampling(self.h, None if sampling is None else C.byref(sampling)))

    def texture_sampling_info(self):
        i = JpTexSamplingInfo()
        i.struct_bytes = C.sizeof(JpTexSamplingInfo)
        self._check(self.lib.jp_get_texture_sampling_info(self.h, C.byref(i)))
        return i

    def set_texture_mipmaps(self, mipmaps):
        """jp_set_texture_mipmaps for the next upload: a JpTextureMipmaps (texture_mipmaps(...) builds one), or None for none"""
        self._check(self.lib.jp_set_texture_mipmaps(self.h, None if mipmaps is None else C.byref(mipmaps)))

    def texture_mipmap_info(self):
        i = JpTextureMipmapInfo()
        i.struct_bytes = C.sizeof(JpTextureMipmapInfo)
        self._check(self.lib.jp_get_texture_mipmap_info(self.h, C.byref(i)))
        return i

    def read_mip_chain(self, texture, w, h):
        """jp_read_mip_chain: the uploaded pyramid of texture `texture` (a w x h image) -> list of (h_k, w_k, 3) uint8 levels, level 0 first"""
        import numpy as np
        sizes = mip_level_sizes(w, h)
        out = np.zeros(3 * sum(a * b for a, b in sizes), np.uint8)
        self._check(self.lib.jp_read_mip_chain(self.h, int(texture), out.ctypes.data_as(C.c_void_p), out.size))
        return _split_chain(out, sizes)

    def mip_probe(self, origin, direction, tmin, tmax, flags, state):
        """jp_mip_probe: closest hit of jp_surface's walk, then k_texel_m's device function on the caller's flags and (n, 2) (width, spread) state
        -> (state after (n, 2), prim (n,), rho (n,), rgb8 (n, 3))"""
        import numpy as np
        n = origin.shape[0]
        o = np.ascontiguousarray(origin, np.float32); d = np.ascontiguousarray(direction, np.float32)
        t0 = np.ascontiguousarray(tmin, np.float32); t1 = np.ascontiguousarray(tmax, np.float32)
        f = np.ascontiguousarray(flags, np.int32); st = np.array(state, np.float32).reshape(n, 2).copy()
        prim = np.zeros(n, np.int32); rho = np.zeros(n, np.float32); rgb = np.zeros((n, 3), np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_mip_probe(self.h, n, p(o), p(d), p(t0), p(t1), p(f), p(st), p(prim), p(rho), p(rgb)))
        return st, prim, rho, rgb

    def set_texture_procedurals(self, procedurals):
        """jp_set_texture_procedurals for the next upload: a JpTextureProcedurals (texture_procedurals(...) builds one), or None for none"""
        self._check(self.lib.jp_set_texture_procedurals(self.h, None if procedurals is None else C.byref(procedurals)))

    def procedural_info(self):
        i = JpProceduralInfo()
        i.struct_bytes = C.sizeof(JpProceduralInfo)
        self._check(self.lib.jp_get_procedural_info(self.h, C.byref(i)))
        return i

    def procedural_probe(self, texture, p, uv, width):
        """jp_procedural_probe: the device twin of procedural_lookup on the uploaded record and colours of texture `texture` -> side words (n,) uint32"""
        import numpy as np
        pp = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        n = pp.shape[0]
        u = np.ascontiguousarray(np.broadcast_to(np.asarray(uv, np.float32), (n, 2)))
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(width, np.float32), (n,)))
        word = np.zeros(n, np.uint32)
        q = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_procedural_probe(self.h, int(texture), n, q(pp), q(u), q(w), q(word)))
        return word

    def shading_normal(self, origin, direction, tmin, tmax):
        """jp_shading_normal: closest hit of jp_trace's walk -> (prim (n,), ng (n, 3), ns (n, 3)): the geometric normal and the shading normal the render uses"""
        import numpy as np
        n = origin.shape[0]
        o = np.ascontiguousarray(origin, np.float32); d = np.ascontiguousarray(direction, np.float32)
        t0 = np.ascontiguousarray(tmin, np.float32); t1 = np.ascontiguousarray(tmax, np.float32)
        prim = np.zeros(n, np.int32); ng = np.zeros((n, 3), np.float32); ns = np.zeros((n, 3), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_shading_normal(self.h, n, p(o), p(d), p(t0), p(t1), p(prim), p(ng), p(ns)))
        return prim, ng, ns

    def synchronize(self):
        self._check(self.lib.jp_synchronize(self.h))

    def set_profiling(self, on):
        self._check(self.lib.jp_set_profiling(self.h, 1 if on else 0))

    def counters(self):
        c = JpCounters()
        self._check(self.lib.jp_get_counters(self.h, C.byref(c)))
        return c

    def build_info(self):
        b = JpBuildInfo()
        self._check(self.lib.jp_get_build_info(self.h, C.byref(b)))
        return b

    def shadow_kernel(self):
        """jp_dbg_shadow_kernel (diagnostic, outside the ABI structs): the shadow kernel the selector picks for the uploaded scene under the options in
        force -> "refill" (a lane-refill kernel), "generic" (k_shadow<mode>), "flat" (k_shadow<2, FeatFlat>) or "pair" (k_shadow_pair)"""
        fn = self.lib.jp_dbg_shadow_kernel
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]; fn.restype = C.c_int
        which = C.c_int(-1)
        self._check(fn(self.h, C.byref(which)))
        return ("refill", "generic", "flat", "pair")[which.value]

    def extend_kernel(self):
        """jp_dbg_extend_kernel (diagnostic, outside the ABI structs): the closest-hit kernel the selector picks for the uploaded scene under the options in
        force -> "refill" (a lane-refill kernel), "generic" (k_extend<mode>), "flat" (k_extend<2, FeatFlat>) or "pool" (k_extend_pool)"""
        fn = self.lib.jp_dbg_extend_kernel
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]; fn.restype = C.c_int
        which = C.c_int(-1)
        self._check(fn(self.h, C.byref(which)))
        return ("refill", "generic", "flat", "pool")[which.value]

    def read_table(self, which):
        """jp_read_scene_table: one hierarchy table of the uploaded scene ("nodes", "prims", "meta", "wide", "q4", "flat"), copied from the device -> uint8 array"""
        return _read_table(lambda out, cap, n: self.lib.jp_read_scene_table(self.h, _table_index(which), out, cap, n))

    def tree_info(self):
        i = JpTreeInfo()
        i.struct_bytes = C.sizeof(JpTreeInfo)
        self._check(self.lib.jp_get_tree_info(self.h, C.byref(i)))
        return i

    def trace(self, origin, direction, tmin, tmax):
        import numpy as np
        n = origin.shape[0]
        o = np.ascontiguousarray(origin, np.float32); d = np.ascontiguousarray(direction, np.float32)
        t0 = np.ascontiguousarray(tmin, np.float32); t1 = np.ascontiguousarray(tmax, np.float32)
        hit = np.zeros(n, np.int32); t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); nrm = np.zeros((n, 3), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_trace(self.h, n, p(o), p(d), p(t0), p(t1), p(hit), p(t), p(prim), p(nrm)))
        return hit, t, prim, nrm

    def occluded(self, origin, direction, tmin, tmax):
        """jp_occluded: the any-hit query of the render's shadow rays -> (occluded int32 (n,), walk): walk is the traversal mode that ran, + 16 for the
        flat-shape instance of the tiny-scene walk"""
        import numpy as np
        n = origin.shape[0]
        o = np.ascontiguousarray(origin, np.float32); d = np.ascontiguousarray(direction, np.float32)
        t0 = np.ascontiguousarray(tmin, np.float32); t1 = np.ascontiguousarray(tmax, np.float32)
        occ = np.zeros(n, np.int32); walk = C.c_int32(-1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_occluded(self.h, n, p(o), p(d), p(t0), p(t1), p(occ), C.byref(walk)))
        return occ, int(walk.value)

    def bsdf(self, desc, normal, wo, wi, u):
        """jp_bsdf: FBSDF::Evalf / Pdf / Sample of a by-value BSDF on the device -> dict of arrays"""
        import numpy as np
        n = normal.shape[0]
        a = [np.ascontiguousarray(x, np.float32) for x in (normal, wo, wi, u)]
        out = dict(f=np.zeros((n, 3), np.float32), pdf=np.zeros(n, np.float32), sf=np.zeros((n, 3), np.float32), swi=np.zeros((n, 3), np.float32),
                   spdf=np.zeros(n, np.float32), sflags=np.zeros(n, np.int32))
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._check(self.lib.jp_bsdf(self.h, C.byref(desc), n, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(out["f"]), p(out["pdf"]), p(out["sf"]), p(out["swi"]), p(out["spdf"]), p(out["sflags"])))
        return out

    def close(self):
        if self.h:
            self.lib.jp_destroy_context(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


from . import scenes  # noqa: E402,F401
from . import distributed  # noqa: E402,F401
