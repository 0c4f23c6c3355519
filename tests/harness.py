"""Test-side bindings: the oracle restatement (oracle/libjp_oracle.so) and, where /root/reference exists, the
compiled reference (oracle/_ref/libjp_ref.so).  TEST INFRASTRUCTURE: the product never imports this."""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
import jet_pbrt_amd as jp  # noqa: E402
from jet_pbrt_amd import scenes  # noqa: E402

ORACLE_PATH = os.path.join(REPO, "oracle", "libjp_oracle.so")
REF_PATH = os.path.join(REPO, "oracle", "_ref", "libjp_ref.so")
GOLDEN = os.path.join(REPO, "tests", "golden")
_fp = C.POINTER(C.c_float)
_vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(_vp)


_oracle = None
_ref = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        L = C.CDLL(ORACLE_PATH)
        L.jp_oracle_render.argtypes = [C.POINTER(jp.JpScene), C.POINTER(jp.JpRenderParams), C.c_int, _vp, C.POINTER(jp.JpCounters)]
        L.jp_oracle_scene_new.restype = _vp
        L.jp_oracle_scene_new.argtypes = [C.POINTER(jp.JpScene)]
        L.jp_oracle_scene_free.argtypes = [_vp]
        L.jp_oracle_trace.argtypes = [_vp, C.c_int] + [_vp] * 9
        L.jp_oracle_tree_dump.argtypes = [_vp, _vp, _vp, _vp, C.c_int]
        L.jp_oracle_set_watertight.argtypes = [C.c_int]
        L.jp_oracle_camera_rays.argtypes = [_vp, C.c_int, _vp, _vp, _vp]
        L.jp_oracle_bsdf.argtypes = [_vp, C.c_int, C.c_int] + [_vp] * 11
        L.jp_oracle_light_sample.argtypes = [_vp, C.c_int, C.c_int] + [_vp] * 7
        L.jp_oracle_li_scripted.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]
        L.jp_oracle_stock_stream.argtypes = [C.c_int, _vp]
        L.jp_oracle_bsdf_direct.argtypes = [C.POINTER(jp.JpBsdfDesc), C.c_int] + [_vp] * 10
        L.jp_oracle_render_features.argtypes = [C.POINTER(jp.JpScene), C.POINTER(jp.JpRenderParams), C.POINTER(JpOracleFeatures), C.c_int, _vp, C.POINTER(jp.JpCounters), _vp]
        L.jp_oracle_render_features_stats.argtypes = L.jp_oracle_render_features.argtypes + [C.POINTER(JpOracleBranchStats)]
        L.jp_oracle_path_features.argtypes = [C.POINTER(jp.JpScene), C.POINTER(jp.JpRenderParams), C.POINTER(JpOracleFeatures), C.c_int, C.c_int, C.c_int, _vp]
        _oracle = L
    return _oracle


class JpOracleMipChain(C.Structure):
    """oracle/pt_features.h: the pyramid of one image as jp_build_mip_chain returns it"""
    _fields_ = [("n_levels", C.c_int32), ("pad", C.c_int32), ("level_w", C.POINTER(C.c_int32)), ("level_h", C.POINTER(C.c_int32)), ("rgb8", C.POINTER(C.c_uint8))]


class JpOracleBranchStats(C.Structure):
    """oracle/pt_features.h: the lookups of a render per branch of sections 18 and 19; the last index is 0: bounce 0, 1: bounce >= 1"""
    _u2 = C.c_uint64 * 2
    _fields_ = [("struct_bytes", C.c_int32), ("pad", C.c_int32),
                ("mip_rho_zero", _u2), ("mip_rho_le1", _u2), ("mip_two_level", (C.c_uint64 * 16) * 2), ("mip_last_level", _u2),
                ("proc_all_one", _u2 * 6), ("proc_partial", _u2 * 6), ("proc_early", _u2 * 6),
                ("checker_plain", _u2), ("checker_filtered", _u2), ("checker_half", _u2), ("word_sum", _u2)]

    def arrays(self):
        """every count as a numpy array, by field name"""
        return {n: np.array(getattr(self, n), np.uint64) for n, _ in self._fields_[2:]}


class JpOracleFeatures(C.Structure):
    """oracle/pt_features.h: the feature state of jp_oracle_render_features; every field optional"""
    _ip = C.POINTER(C.c_int32)
    _fields_ = [("struct_bytes", C.c_int32), ("light_mode", C.c_int32), ("n_lights", C.c_int32), ("n_env", C.c_int32),
                ("q", _fp), ("alias", _ip), ("pmf", _fp), ("env_lights", _ip),
                ("env_w", C.c_int32), ("env_h", C.c_int32), ("env_up", C.c_int32), ("env_light", C.c_int32),
                ("env_texel", _fp), ("env_q", _fp), ("env_alias", _ip), ("env_row_cos", _fp),
                ("estimator", C.c_int32), ("watertight", C.c_int32),
                ("normals", C.POINTER(jp.JpVertexNormals)), ("textures", C.POINTER(jp.JpTextures)), ("sampling", C.POINTER(jp.JpTextureSampling)),
                ("normal_maps", C.POINTER(jp.JpNormalMaps)), ("lens", C.POINTER(jp.JpLens)), ("film", C.POINTER(jp.JpFilm)),
                ("mipmaps", C.POINTER(jp.JpTextureMipmaps)), ("n_mip_chains", C.c_int32), ("pad0", C.c_int32), ("mip_chains", C.POINTER(JpOracleMipChain)),
                ("procedurals", C.POINTER(jp.JpTextureProcedurals))]


def _scene_arr(p, n, dt=np.float32):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy() if n else np.zeros(0, dt)


def light_weights(s, env_mean_sum=None):
    """INTEGRATION.md section 9 "Weights": one double per light of the JpScene `s`, from the fp32 scene values; areas in fp32 with the upload's expressions
    (shape.h:351, 457, 546, 253).  env_mean_sum: the scene's one environment light carries a map, whose mean_sum takes the radiance sum's place (section 10)."""
    f32 = np.float32
    n = s.n_lights
    ty = _scene_arr(s.light_type, n, np.int32); rad = _scene_arr(s.light_radiance, 3 * n).reshape(n, 3).astype(np.float64); lp = _scene_arr(s.light_prim, n, np.int32)
    st, si = _scene_arr(s.prim_shape_type, s.n_primitives, np.int32), _scene_arr(s.prim_shape_index, s.n_primitives, np.int32)
    T = [_scene_arr(getattr(s, "tri_p%d" % k), 3 * s.n_triangles).reshape(-1, 3) for k in range(3)]
    Q = [_scene_arr(getattr(s, "rect_p%d" % k), 3 * s.n_rectangles).reshape(-1, 3) for k in range(3)]
    sr = _scene_arr(s.sph_radius, s.n_spheres); dr = _scene_arr(s.disk_radius, s.n_disks)
    kpi = f32(3.14159265358979323846)

    def cross_len(a, b):
        a = a.astype(f32); b = b.astype(f32)
        c = [f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])]
        return np.sqrt(f32(f32(c[0] * c[0]) + f32(c[1] * c[1])) + f32(c[2] * c[2]), dtype=f32)
    R2 = float(s.world_radius) * float(s.world_radius)
    w = np.zeros(n)
    for i in range(n):
        ssum = (rad[i, 0] + rad[i, 1]) + rad[i, 2]
        if ty[i] == 1:                                                  # JP_LIGHT_AREA
            p = lp[i]; k = si[p]
            if st[p] == 0:
                area = f32(0.5) * cross_len(T[1][k] - T[0][k], T[2][k] - T[0][k])
            elif st[p] == 1:
                area = cross_len(Q[0][k] - Q[1][k], Q[2][k] - Q[1][k])
            elif st[p] == 3:                                            # JP_SHAPE_DISK
                area = f32(f32(kpi * dr[k]) * dr[k])
            else:
                area = f32(f32(f32(4) * kpi) * f32(sr[k] * sr[k]))
            w[i] = (ssum * float(area)) * np.pi
        elif ty[i] == 2:                                                # JP_LIGHT_POINT
            w[i] = ssum * (4.0 * np.pi)
        elif ty[i] == 0 and env_mean_sum is not None:                   # the map light
            w[i] = (env_mean_sum * np.pi) * R2
        else:
            w[i] = (ssum * np.pi) * R2
    return w


def _as_ptr(x, ty):
    """a ctypes pointer to `x`: None, an instance of ty, or already a pointer (what HostBackend.flatten_* return)"""
    if x is None:
        return None, None
    if isinstance(x, C._Pointer):
        return x, x
    return C.pointer(x), x


def texture_images(textures):
    """the images of a JpTextures (or a pointer to one): {texture index: (h, w, 3) uint8 array}"""
    t = textures.contents if isinstance(textures, C._Pointer) else textures
    out = {}
    for k in range(t.n_textures):
        if t.tex_type[k] == jp.JP_TEXTURE_IMAGE:
            w, h = t.tex_width[k], t.tex_height[k]
            out[k] = np.ctypeslib.as_array(C.cast(t.texels, C.POINTER(C.c_uint8)), shape=(t.n_texel_bytes,))[t.tex_offset[k]:t.tex_offset[k] + 3 * w * h].reshape(h, w, 3).copy()
    return out


def mip_chains(textures, mipmaps):
    """the JpOracleMipChain array of a JpTextures under a JpTextureMipmaps: jp_build_mip_chain's arrays (pure host code with tests of its own) for every image
    whose mode is TRILINEAR -> (ctypes array, keep-alive list)"""
    t = textures.contents if isinstance(textures, C._Pointer) else textures
    m = mipmaps.contents if isinstance(mipmaps, C._Pointer) else mipmaps
    arr = (JpOracleMipChain * max(1, t.n_textures))()
    keep = []
    for k, img in texture_images(t).items():
        if not m.mode or m.mode[k] != jp.JP_MIP_TRILINEAR:
            continue
        levels = jp.build_mip_chain(img)
        lw = np.array([l.shape[1] for l in levels], np.int32); lh = np.array([l.shape[0] for l in levels], np.int32)
        flat = np.ascontiguousarray(np.concatenate([l.reshape(-1) for l in levels]), np.uint8)
        arr[k] = JpOracleMipChain(len(levels), 0, lw.ctypes.data_as(C.POINTER(C.c_int32)), lh.ctypes.data_as(C.POINTER(C.c_int32)), flat.ctypes.data_as(C.POINTER(C.c_uint8)))
        keep += [lw, lh, flat]
    return arr, keep


def oracle_features(scene_ptr, light_mode=None, env_rgb=None, env_up="z", env_importance=0, estimator=None, normals=None, textures=None, sampling=None,
                    normal_maps=None, lens=None, film=None, watertight=False, mipmaps=None, procedurals=None):
    """The JpOracleFeatures of a feature set, built the way the library builds its state: light_mode "power" takes the light table from
    jp_build_light_table over light_weights(); env_rgb (an (H, W, 3) array) the map tables from jp_build_environment_table with the scene's one environment
    light as the tint.  The other arguments are the structs the Context setters take (or pointers to them).  Everything is kept alive on the result."""
    s = scene_ptr.contents
    f = JpOracleFeatures()
    f.struct_bytes = C.sizeof(JpOracleFeatures)
    keep = []
    ip = C.POINTER(C.c_int32)
    mean_sum = None
    if env_rgb is not None:
        ty = _scene_arr(s.light_type, s.n_lights, np.int32); rad = _scene_arr(s.light_radiance, 3 * s.n_lights).reshape(-1, 3)
        at = [i for i in range(s.n_lights) if ty[i] == 0]
        assert len(at) == 1, "a map needs exactly one environment light"
        e = jp.build_environment_table(env_rgb, tuple(rad[at[0]]), env_up, env_importance)
        f.env_h, f.env_w = np.asarray(env_rgb).shape[:2]; f.env_up = jp.ENV_UP_AXES[env_up]; f.env_light = at[0]
        f.env_texel = e["texel"].ctypes.data_as(_fp); f.env_q = e["q"].ctypes.data_as(_fp); f.env_alias = e["alias"].ctypes.data_as(ip); f.env_row_cos = e["row_cos"].ctypes.data_as(_fp)
        keep.append(e); mean_sum = e["mean_sum"]
    f.light_mode = jp.LIGHT_SAMPLING_MODES[light_mode]
    if f.light_mode == jp.JP_LIGHTS_POWER_ONE:
        w = light_weights(s, mean_sum)
        q, alias, pmf = jp.build_light_table(w)
        ty = _scene_arr(s.light_type, s.n_lights, np.int32); rad = _scene_arr(s.light_radiance, 3 * s.n_lights).reshape(-1, 3)
        envl = np.array([i for i in range(s.n_lights) if ty[i] == 0 and (rad[i] != 0).any()], np.int32)
        f.n_lights = s.n_lights; f.q = q.ctypes.data_as(_fp); f.alias = alias.ctypes.data_as(ip); f.pmf = pmf.ctypes.data_as(_fp)
        f.n_env = len(envl); f.env_lights = envl.ctypes.data_as(ip) if len(envl) else None
        keep += [w, q, alias, pmf, envl]
        f.table = (w, q, alias, pmf)
    f.estimator = jp.ESTIMATOR_MODES[estimator]
    f.watertight = 1 if watertight else 0
    for name, val, ty in (("normals", normals, jp.JpVertexNormals), ("textures", textures, jp.JpTextures), ("sampling", sampling, jp.JpTextureSampling),
                          ("normal_maps", normal_maps, jp.JpNormalMaps), ("lens", lens, jp.JpLens), ("film", film, jp.JpFilm),
                          ("mipmaps", mipmaps, jp.JpTextureMipmaps), ("procedurals", procedurals, jp.JpTextureProcedurals)):
        p, k = _as_ptr(val, ty)
        if p is not None:
            setattr(f, name, C.cast(p, C.POINTER(ty))); keep.append((p, k))
    if mipmaps is not None and textures is not None:                # the pyramids as data: jp_build_mip_chain's arrays
        arr, k2 = mip_chains(textures, mipmaps)
        f.n_mip_chains = len(arr); f.mip_chains = C.cast(arr, C.POINTER(JpOracleMipChain)); keep += [arr, k2]
    f._keep = keep
    return f


def oracle_render_features(scene_ptr, params, features=None, nthreads=8, rand_seed=1, stats=None):
    """jp_oracle_render_features -> (film, JpCounters, undecided (H, W) bool).  features: oracle_features(...) or None.  rand_seed: as oracle_render.
    stats: a JpOracleBranchStats to fill (jp_oracle_render_features_stats)."""
    film = np.zeros((params.height, params.width, 3), np.float32)
    und = np.zeros((params.height, params.width), np.uint8)
    cnt = jp.JpCounters()
    L = oracle_lib()
    if rand_seed is not None:
        libc_srand(rand_seed)
    if stats is not None:
        stats.struct_bytes = C.sizeof(JpOracleBranchStats)
        st = L.jp_oracle_render_features_stats(scene_ptr, C.byref(params), None if features is None else C.byref(features), nthreads, ptr(film), C.byref(cnt), ptr(und), C.byref(stats))
    else:
        st = L.jp_oracle_render_features(scene_ptr, C.byref(params), None if features is None else C.byref(features), nthreads, ptr(film), C.byref(cnt), ptr(und))
    if st != 0:
        raise jp.JetPbrtError("jp_oracle_render_features: status %d" % st)
    return film, cnt, und.astype(bool)


def oracle_path_features(scene_ptr, params, features, x, y, s, rand_seed=1):
    """jp_oracle_path_features: sample s of pixel (x, y) alone, its draws, decisions and contributions printed to stdout -> the sample's radiance"""
    out = np.zeros(3, np.float32)
    if rand_seed is not None:
        libc_srand(rand_seed)
    st = oracle_lib().jp_oracle_path_features(scene_ptr, C.byref(params), None if features is None else C.byref(features), x, y, s, ptr(out))
    if st != 0:
        raise jp.JetPbrtError("jp_oracle_path_features: status %d" % st)
    return out


def have_ref():
    return os.path.exists(REF_PATH)


def ref_lib():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_PATH)
        L.ref_scene_new.restype = _vp
        L.ref_scene_new.argtypes = [C.c_char_p]
        L.ref_scene_free.argtypes = [_vp]
        L.ref_scene_camera.argtypes = [_vp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float]
        L.ref_scene_envlight.argtypes = [_vp, _fp]
        L.ref_scene_pointlight.argtypes = [_vp, _fp, _fp]
        L.ref_scene_dirlight.argtypes = [_vp, _fp, _fp]
        L.ref_mat_matte.argtypes = [_vp, _fp]
        L.ref_mat_mirror.argtypes = [_vp, _fp]
        L.ref_mat_glass.argtypes = [_vp, C.c_float, _fp, _fp]
        L.ref_mat_plastic.argtypes = [_vp, _fp, _fp, C.c_float, C.c_int]
        L.ref_mat_metal.argtypes = [_vp, _fp, _fp, C.c_float, C.c_float, C.c_int]
        L.ref_scene_mesh.argtypes = [_vp, C.c_char_p, C.c_int, C.c_int, _fp, C.c_float, C.c_int, _fp]
        L.ref_scene_rect.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _fp]
        L.ref_scene_sphere.argtypes = [_vp, _fp, C.c_float, C.c_int, _fp]
        L.ref_scene_disk.argtypes = [_vp, _fp, _fp, C.c_float, C.c_int, _fp]
        L.ref_scene_preprocess.argtypes = [_vp]
        L.ref_num_primitives.argtypes = [_vp]
        L.ref_num_lights.argtypes = [_vp]
        L.ref_render.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, _vp]
        L.ref_render_recursive.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, _vp]
        L.ref_render_other.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, _vp]
        L.ref_counters_reset.argtypes = [_vp]
        L.ref_counters_get.argtypes = [_vp, _vp]
        L.ref_trace.argtypes = [_vp, C.c_int] + [_vp] * 9
        L.ref_camera_rays.argtypes = [_vp, C.c_int, _vp, _vp, _vp]
        L.ref_bsdf.argtypes = [_vp, C.c_int, C.c_int] + [_vp] * 11
        L.ref_light_sample.argtypes = [_vp, C.c_int, C.c_int] + [_vp] * 7
        L.ref_li_scripted.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]
        L.ref_stock_stream.argtypes = [C.c_int, _vp]
        L.ref_stock_float2.argtypes = [_vp]
        L.ref_bsdf_direct.argtypes = [C.POINTER(jp.JpBsdfDesc), C.c_int] + [_vp] * 10
        L.ref_film_save.argtypes = [_vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.ref_gamma_encode.argtypes = [_vp, C.c_int, _vp]
        _ref = L
    return _ref


class RefBackend(scenes.HostBackend):
    """The same procedural scene API over the compiled, unmodified reference."""
    prefix = "ref_"

    def __init__(self, name="scene"):
        super().__init__(name, lib=ref_lib())

    def _new(self, name):
        self.h = C.c_void_p(self.L.ref_scene_new(name.encode()))

    rand_seed = 1

    def preprocess(self):
        """FScene::Preprocess (scene.cc:11-23) grows the tree from libc rand(): from the state a fresh reference process has, whatever this process did before
        (oracle_render; set rand_seed = None on the instance to leave the state alone)"""
        if self.rand_seed is not None:
            libc_srand(self.rand_seed)
        super().preprocess()

    def render(self, W, H, spp, maxdepth=5, sampler_mode=1, seed=1234, nthreads=8):
        film = np.zeros((H, W, 3), np.float32)
        st = self.L.ref_render(self.h, W, H, spp, maxdepth, sampler_mode, seed, nthreads, ptr(film))
        assert st == 0
        return film

    def render_recursive(self, W, H, spp, maxdepth=5, seed=1234):
        """the reference's FPathIntegratorRecursive (integrator.cc:233-307), counter sampler, serial"""
        film = np.zeros((H, W, 3), np.float32)
        st = self.L.ref_render_recursive(self.h, W, H, spp, maxdepth, seed, ptr(film))
        assert st == 0
        return film

    def render_other(self, kind, W, H, spp, maxdepth=5, seed=1234):
        """the reference's FWhittedIntegrator (kind 1) / FDebugIntegrator (kind 2), counter sampler, serial"""
        film = np.zeros((H, W, 3), np.float32)
        st = self.L.ref_render_other(self.h, kind, W, H, spp, maxdepth, seed, ptr(film))
        assert st == 0
        return film

    def counters(self):
        out = np.zeros(4, np.uint64)
        self.L.ref_counters_get(self.h, ptr(out))
        return out


def oracle_render(scene_ptr, params, nthreads=8, watertight=False, rand_seed=1):
    """watertight=True: the reference's arithmetic with a conservative box test (oracle/pt_oracle.cc box_hit), i.e. without
    the hits the reference's own BVH drops on finely tessellated meshes.
    rand_seed: the oracle rebuilds the reference's BVH, whose split axes come from libc rand() (bvh.h:61); every render starts from the state a fresh
    reference process has (srand(1)), so that a film on a mesh -- where the hits in the fp32 acceptance fringe depend on that tree -- does not depend on how many
    trees this process has built before -- nor on the HIP runtime: libamd_comgr calls srand() with a seed of its own and rand() whenever it loads a code object
    (tools/randtrace: 66 calls and one srand in the main thread of a GPU test run), which used to make every later un-seeded oracle tree a different one per run.  None: leave the state alone (tools that sweep it)."""
    film = np.zeros((params.height, params.width, 3), np.float32)
    cnt = jp.JpCounters()
    L = oracle_lib()
    if rand_seed is not None:
        libc_srand(rand_seed)
    L.jp_oracle_set_watertight(1 if watertight else 0)
    try:
        st = L.jp_oracle_render(scene_ptr, C.byref(params), nthreads, ptr(film), C.byref(cnt))
    finally:
        L.jp_oracle_set_watertight(0)
    assert st == 0
    return film, cnt


SCENES = {
    "cornell": lambda be, W, H: scenes.build_cornell(be, W, H, lambert_only=False),
    "cornell_lambert": lambda be, W, H: scenes.build_cornell(be, W, H, lambert_only=True),
    # the committed OBJ fixture (numpy's sin/cos may differ in the last bit between hosts; the goldens must not)
    "bunny_small": lambda be, W, H: scenes.build_bunny(be, W, H, obj_path=os.path.join(GOLDEN, "bunny_24x16.obj")),
    "misc": lambda be, W, H: scenes.build_misc(be, W, H),
    "lights": lambda be, W, H: scenes.build_lights(be, W, H),
    "disks": lambda be, W, H: scenes.build_disks(be, W, H),
}


def build_random_scene(be, W, Hh, seed, n_tris=120, tmpdir=None):
    """Random triangle soup + rectangles + spheres, every material kind, triangle / rectangle / sphere area lights and
    a coloured environment -- the same call sequence on any backend."""
    import tempfile
    rng = np.random.default_rng(seed)
    d = tmpdir or tempfile.mkdtemp(prefix="jp_rand_")
    be.camera((0, 0, 9), (0, 0, -1), (0, 1, 0), 55.0, W, Hh)
    be.envlight(tuple(float(v) for v in rng.uniform(0.0, 0.3, 3)))
    mats = [be.mat_matte(tuple(rng.uniform(0.1, 0.9, 3))), be.mat_matte(tuple(rng.uniform(0.1, 0.9, 3))),
            be.mat_metal(tuple(rng.uniform(0.1, 1.5, 3)), tuple(rng.uniform(0.1, 3.0, 3)), float(rng.uniform(0.05, 0.4)), float(rng.uniform(0.05, 0.4)), bool(rng.integers(0, 2))),
            be.mat_plastic(tuple(rng.uniform(0.1, 0.6, 3)), tuple(rng.uniform(0.1, 0.4, 3)), float(rng.uniform(0.05, 0.5)), bool(rng.integers(0, 2))),
            be.mat_glass(float(rng.uniform(1.2, 1.8)), (0.95, 0.95, 0.95), (0.9, 0.95, 0.9)), be.mat_mirror((0.85, 0.85, 0.9))]
    # four soups with different materials
    for m in range(4):
        c = rng.uniform(-3, 3, (n_tris // 4, 1, 3)); v = (c + rng.normal(0, 0.7, (n_tris // 4, 3, 3))).reshape(-1, 3).astype(np.float32)
        f = np.arange(v.shape[0]).reshape(-1, 3)
        path = os.path.join(d, "soup_%d_%d.obj" % (seed, m))
        scenes.write_obj(path, v, f)
        be.mesh(path, bool(m & 1), bool(m & 2), (0, 0, -1.0 * m), 1.0, mats[m], None)
    # a mesh light (two triangles), a rectangle light and a sphere light
    lp = os.path.join(d, "light_%d.obj" % seed)
    scenes.write_obj(lp, np.array([[-1, 3.9, -1], [1, 3.9, -1], [1, 3.9, 1], [-1, 3.9, 1]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]))
    be.mesh(lp, False, False, (0, 0, 0), 1.0, mats[0], tuple(rng.uniform(5, 20, 3)))
    be.rect(scenes.AXIS_YZ, -1, 1, -2, 0, -4.0, False, mats[1], tuple(rng.uniform(2, 8, 3)))
    be.sphere((2.5, 2.0, 1.0), 0.5, mats[0], tuple(rng.uniform(5, 15, 3)))
    be.sphere((-1.5, -1.0, 1.5), 0.8, mats[4], None)
    be.sphere((1.2, -1.5, 0.5), 0.6, mats[5], None)
    be.rect(scenes.AXIS_XZ, -6, 6, -6, 6, -3.0, False, mats[1], None)
    be.rect(scenes.AXIS_XY, -6, 6, -3, 5, -6.0, False, mats[3], None)
    be.preprocess()
    return be


def oracle_scene(L, scene_ptr, rand_seed=1):
    """jp_oracle_scene_new from the rand() state of a fresh reference process (see oracle_render)"""
    if rand_seed is not None:
        libc_srand(rand_seed)
    return L.jp_oracle_scene_new(scene_ptr)


def libc_srand(seed=1):
    """the reference BVH draws its split axes from libc rand() (bvh.h:61); reset it so that the compiled
    reference and the restatement build the same tree."""
    C.CDLL(None).srand(seed)


def bsdf_cases():
    """the by-value BSDFs of the KAT set (tests/golden/kat_bsdf.npz): every class of bsdf.h / microfacet.h, the ones no material builds included"""
    D = jp.bsdf_desc
    return {
        "lambert": D(jp.JP_BSDF_LAMBERT, color=(0.63, 0.065, 0.05)),
        "mirror": D(jp.JP_BSDF_MIRROR, color=(0.9, 0.85, 0.8)),
        "fresnel_specular": D(jp.JP_BSDF_FRESNEL_SPECULAR, color=(0.98, 0.97, 0.96), color2=(0.95, 0.96, 0.97), eta_a=1.0, eta_b=1.5),
        "phong_20": D(jp.JP_BSDF_PHONG, color=(0.7, 0.6, 0.5), exponent=20.0),
        "phong_3": D(jp.JP_BSDF_PHONG, color=(0.2, 0.9, 0.4), exponent=3.0),
        "tr_conductor": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(1, 1, 1), distribution=0, alpha=(0.2, 0.2), fresnel=0, fr_eta_i=(1, 1, 1), fr_eta_t=(0.18, 0.15, 0.81), fr_k=(0.11, 0.11, 0.11)),
        "tr_noop_aniso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.8, 0.7, 0.9), distribution=0, alpha=(0.15, 0.4), fresnel=2),
        "tr_full_iso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.8, 0.8, 0.8), distribution=0, alpha=(0.3, 0.3), sample_visible=False, fresnel=1, fr_eta_i=(1.0,) * 3, fr_eta_t=(1.5,) * 3),
        "tr_full_aniso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.8, 0.8, 0.8), distribution=0, alpha=(0.1, 0.35), sample_visible=False, fresnel=2),
        "beck_conductor": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(1, 1, 1), distribution=1, alpha=(0.25, 0.25), fresnel=0, fr_eta_i=(1.2, 1.1, 1.0), fr_eta_t=(0.2, 0.9, 1.1), fr_k=(3.9, 2.4, 2.2)),
        "beck_dielectric_aniso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.9, 0.9, 0.9), distribution=1, alpha=(0.12, 0.3), fresnel=1, fr_eta_i=(1.5,) * 3, fr_eta_t=(1.0,) * 3),
        "beck_full_iso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.7, 0.7, 0.7), distribution=1, alpha=(0.2, 0.2), sample_visible=False, fresnel=2),
        "beck_full_aniso": D(jp.JP_BSDF_MICROFACET_REFLECTION, color=(0.7, 0.7, 0.7), distribution=1, alpha=(0.4, 0.1), sample_visible=False, fresnel=2),
        "trans_tr": D(jp.JP_BSDF_MICROFACET_TRANSMISSION, color=(0.95, 0.9, 0.85), distribution=0, alpha=(0.2, 0.2), eta_a=1.0, eta_b=1.5),
        "trans_beck": D(jp.JP_BSDF_MICROFACET_TRANSMISSION, color=(0.9, 0.95, 1.0), distribution=1, alpha=(0.3, 0.15), eta_a=1.0, eta_b=1.33),
        "trans_tr_full": D(jp.JP_BSDF_MICROFACET_TRANSMISSION, color=(1, 1, 1), distribution=0, alpha=(0.25, 0.25), sample_visible=False, eta_a=1.5, eta_b=1.0),
    }


def bsdf_inputs(n, seed):
    """shading events: unit normals, wo / wi spread over both hemispheres (a third of the wi on the far side: transmission), grazing and
    normal incidence included, u in [0, 1)^2 with a few extreme values"""
    rng = np.random.default_rng(seed)
    def unit(v): return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    nrm = unit(rng.normal(size=(n, 3)))
    wo = unit(rng.normal(size=(n, 3))); wi = unit(rng.normal(size=(n, 3)))
    same = rng.random(n) < 0.66
    so = np.sign((wo * nrm).sum(1)); si = np.sign((wi * nrm).sum(1))
    flip = np.where(same, so * si < 0, so * si > 0)
    wi = np.where(flip[:, None], wi - 2 * (wi * nrm).sum(1, keepdims=True) * nrm, wi).astype(np.float32)
    wo[:8] = unit(nrm[:8] + 1e-3 * rng.normal(size=(8, 3)))            # normal incidence
    u = rng.random((n, 2)).astype(np.float32)
    u[:4] = [[0.0, 0.0], [0.999999, 0.5], [0.5, 0.999999], [1e-7, 0.25]]
    return nrm, unit(wo), unit(wi), u


def run_bsdf(fn, desc, nrm, wo, wi, u):
    n = nrm.shape[0]
    out = dict(f=np.zeros((n, 3), np.float32), pdf=np.zeros(n, np.float32), sf=np.zeros((n, 3), np.float32), swi=np.zeros((n, 3), np.float32),
               spdf=np.zeros(n, np.float32), sflags=np.zeros(n, np.int32))
    fn(C.byref(desc), n, ptr(nrm), ptr(wo), ptr(wi), ptr(u), ptr(out["f"]), ptr(out["pdf"]), ptr(out["sf"]), ptr(out["swi"]), ptr(out["spdf"]), ptr(out["sflags"]))
    return out
