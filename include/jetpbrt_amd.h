/* include/jetpbrt_amd.h -- C ABI of the MI355X path-tracing integrator (libjetpbrt_amd.so).
 *
 * Drop-in boundary.  The reference has no FFI; the seam this library sits behind is
 *     void FIntegrator::Render(const FScene*, FSampler*, FFilm*, int numthreads) const   (integrator.h:32,
 *     integrator.cc:35-80)  with  FPathIntegratorIteration::Li  (integrator.cc:316-403)  as the integrator.
 * A host `Render()` (ours: jet-pbrt_amd/host/integrator.h, FGpuPathIntegrator::Render) flattens the
 * preprocessed FScene into the plain arrays of JpScene and calls the entry points below instead of spawning
 * the 20-row CPU tasks of integrator.cc:53-74 / parallel.cc.
 *
 * Conventions: plain C types only; every function returns JP_OK (0) or a negative JpStatus and never throws;
 * jp_last_error() returns a thread-local message for the last failure.  The caller owns every host buffer;
 * the context owns all device memory.  All floats are IEEE binary32 ("Float" = float, pbrt.h:27).
 * Arrays of points/vectors/colours are tightly packed xyz / rgb triples.
 */
#ifndef JETPBRT_AMD_H
#define JETPBRT_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JP_ABI_VERSION 7

typedef enum JpStatus {
    JP_OK = 0,
    JP_ERR_INVALID_ARGUMENT = -1,   /* null pointer, bad enum, index out of range, malformed BVH ... */
    JP_ERR_NO_DEVICE = -2,          /* no HIP device / device id out of range                         */
    JP_ERR_DEVICE = -3,             /* a HIP runtime call failed (message has the hipError string)    */
    JP_ERR_NO_SCENE = -4,           /* jp_render before jp_upload_scene                               */
    JP_ERR_UNSUPPORTED = -5         /* e.g. sampler mode the device path cannot reproduce             */
} JpStatus;

/* shape kinds: FTriangle shape.h:277-369, FRectangle shape.h:380-472, FSphere shape.h:476-662, FDisk shape.h:189-275 */
enum { JP_SHAPE_TRIANGLE = 0, JP_SHAPE_RECTANGLE = 1, JP_SHAPE_SPHERE = 2, JP_SHAPE_DISK = 3 };
/* material kinds: material.h:27-41 (matte), :45-59 (mirror), :63-81 (glass), :85-110 + material.cc:12-29
 * (plastic), material.h:113-137 + material.cc:31-43 (metal) */
enum { JP_MAT_MATTE = 0, JP_MAT_MIRROR = 1, JP_MAT_GLASS = 2, JP_MAT_PLASTIC = 3, JP_MAT_METAL = 4 };
/* light kinds: FEnvironmentLight light.h:248-311, FAreaLight light.h:183-244, FPointLight light.h:81-132,
 * FDirectionLight light.h:136-180 */
enum { JP_LIGHT_ENVIRONMENT = 0, JP_LIGHT_AREA = 1, JP_LIGHT_POINT = 2, JP_LIGHT_DIRECTION = 3 };
/* sampler: the stock sequential mt19937_64 stream (sampler.h:16-54) cannot be reproduced by a parallel
 * device; the device path implements the counter-based stream of include/jp_counter_rng.h only. */
enum { JP_SAMPLER_STOCK_MT19937 = 0, JP_SAMPLER_COUNTER = 1,
       JP_SAMPLER_DEBUG = 2 };  /* FDebugSampler sampler.h:109-127: every draw is 0.5, the camera sample is the pixel + (0.5, 0.5) (what the body of its
                                 * GetCameraSample computes; the reference's function lacks its return statement)                                  */
/* integrators (integrator.h): PATH = FPathIntegratorIteration (integrator.cc:316-403; FPathIntegratorRecursive is the same
 * estimator); WHITTED = FWhittedIntegrator (integrator.cc:115-220; branches at mirrors, one thread walks a sample's whole
 * tree); DEBUG_NORMAL = FDebugIntegrator (integrator.h:44-58).  The last two are API completeness, not the hot path. */
enum { JP_INTEGRATOR_PATH = 0, JP_INTEGRATOR_WHITTED = 1, JP_INTEGRATOR_DEBUG_NORMAL = 2 };

#define JP_MAT_PARAM_STRIDE 16
/* mat_params layout, JP_MAT_PARAM_STRIDE floats per material (the state the reference material objects hold):
 *   MATTE   [0..2] diffuseColor                                                     material.h:29-40
 *   MIRROR  [0..2] specularColor                                                    material.h:47-58
 *   GLASS   [0] eta, [1..3] Kr, [4..6] Kt                                           material.h:65-80
 *   PLASTIC [0..2] Kd, [3..5] Ks, [6] alpha (roughness after the optional remap), [7] Qd      material.h:88-109
 *   METAL   [0..2] eta, [3..5] k, [6] alpha_x, [7] alpha_y (after the optional remap)         material.h:116-136
 */

/* FCamera state after its constructor (camera.h:36-49): right/up already scaled by tan(fov/2) (and aspect). */
typedef struct JpCamera {
    float pos[3], front[3], right[3], up[3];
    float res_x, res_y;
} JpCamera;

typedef struct JpScene {
    JpCamera camera;

    /* shapes, SoA */
    int32_t n_triangles;   const float *tri_p0, *tri_p1, *tri_p2, *tri_n;              /* n = FTriangle::normal (flip applied) */
    int32_t n_rectangles;  const float *rect_p0, *rect_p1, *rect_p2, *rect_p3, *rect_n;
    int32_t n_spheres;     const float *sph_center; const float *sph_radius;

    /* primitives (FPrimitive, primitive.h:20-64) in creation order == FScene::shadow_primitives before Preprocess */
    int32_t n_primitives;
    const int32_t *prim_shape_type;    /* JP_SHAPE_*                                    */
    const int32_t *prim_shape_index;   /* index into the arrays of that shape kind      */
    const int32_t *prim_material;      /* material index, -1 = nullptr material         */
    const int32_t *prim_light;         /* index into lights (FPrimitive::arealight), -1 = none */

    int32_t n_materials;   const int32_t *mat_type; const float *mat_params;

    /* lights in FScene::Lights() order (creation order; scene.h:92-106) */
    int32_t n_lights;
    const int32_t *light_type;         /* JP_LIGHT_*                                    */
    const float   *light_radiance;     /* rgb: radiance (AREA, ENVIRONMENT), intensity (POINT), irradiance (DIRECTION) */
    const int32_t *light_prim;         /* AREA: primitive whose shape emits; otherwise -1 */
    const float   *light_vec;          /* xyz per light: POINT worldPosition, DIRECTION normalised worldDir, otherwise 0;
                                          may be NULL when the scene has neither kind */
    float world_radius;                /* FEnvironmentLight / FDirectionLight::worldRadius after Preprocess (light.cc:17-33) */

    /* bounding volume hierarchy over the primitives, built by the host (own topology; closest-hit and
     * occlusion results do not depend on it).  Node i: bounds 6 floats (min xyz, max xyz);
     * bvh_left[i] >= 0: interior, children bvh_left[i], bvh_right[i];
     * bvh_left[i] <  0: leaf, primitives bvh_prim_index[first .. first+count) with first = -bvh_left[i]-1,
     *                   count = bvh_right[i].  Node 0 is the root.
     * n_bvh_nodes == 0 (all four pointers may be NULL): no hierarchy is handed over and jp_upload_scene builds one on
     * the device from the primitive extents (LBVH; replaces the host build of FScene::Preprocess, scene.cc:11-23). */
    int32_t n_bvh_nodes;   const float *bvh_bounds; const int32_t *bvh_left, *bvh_right;
    int32_t n_bvh_prim_indices; const int32_t *bvh_prim_index;
    /* 0: the hierarchy is acceleration only -- the library is free to re-shape it (8-wide shadow tree, flat leaf list) and
     *    tests boxes conservatively, so no hit is ever dropped.
     * 1: REFERENCE SEMANTICS -- the given tree is walked node for node the way FBVH_Node::Intersect does (bvh.h:94-103: box
     *    test of geometry.cc:10-30 with its `tmax <= tmin` rejection on the unpadded bounds, left subtree then right, leaf
     *    objects in order).  With the reference's own tree (host: FScene::referenceTree) the hits are then the reference's hits
     *    even where those depend on its topology (finely tessellated meshes, DESIGN.md "Numerics").  Several times slower.
     * 2: (ABI 6) REFERENCE SEMANTICS, CERTIFIED WALK -- scenes of more than 1024 primitives: the rays take an ordered walk over the LEAVES
     *    of the given tree; each result carries a proof that the walk of (1) returns the same hit (FBounds3::Intersect on the hit's leaf
     *    box with max_t = the hit distance implies the same for every ancestor and every larger max_t), and the rays without a proof are
     *    walked again as in (1).  About twice as fast as (1).  One class of rays is outside the proof: a ray within fp32 noise of a
     *    triangle's plane is accepted or not by the signs of rounding errors, wherever along the ray that triangle lies.  Rays from the camera
     *    position are covered (leaves with a primitive edge-on to the camera are never culled by distance for them); for secondary rays there is
     *    only a generous distance-cull slack and the measurement: the 280k-triangle frame at 800x600x2048 and a 1/8 shard of 1920x1080x4096 are bit-identical
     *    to (1) (DESIGN.md "Certified walk").  Smaller scenes: as (1). */
    int32_t bvh_reference_semantics;

    /* FDisk (shape.h:189-275): position, normal (already normalised by the constructor, shape.h:194), radius */
    int32_t n_disks;       const float *disk_center, *disk_normal; const float *disk_radius;
} JpScene;

typedef struct JpRenderParams {
    int32_t width, height;       /* film size == camera resolution (main.cc:115)                          */
    int32_t spp;                 /* FSampler::samples_per_pixel                                           */
    int32_t max_depth;           /* FPathIntegratorIteration::maxDepth (main.cc:154: 5)                   */
    int32_t sampler_mode;        /* JP_SAMPLER_*                                                          */
    uint32_t seed;               /* counter sampler seed                                                  */
    /* pixel-band sharding (multi-GPU): the film is cut into bands of `band_rows` rows -- the unit of
     * FRenderTask, lines_per_task = 20, integrator.cc:53 -- and this call renders band b iff
     * b % shard_count == shard_index.  Pixels outside the shard are written as 0, so the sum over shards
     * (one RCCL reduce) is the full film.  shard_count <= 1 renders everything. */
    int32_t band_rows, shard_index, shard_count;
    int32_t integrator;          /* JP_INTEGRATOR_*: 0 = FPathIntegratorIteration / Recursive (the hot path, wavefront kernels)   */
} JpRenderParams;

typedef struct JpCounters {
    uint64_t samples;            /* camera samples traced                                                 */
    uint64_t closest_rays;       /* FScene::Intersect calls from Li (integrator.cc:327)                   */
    uint64_t closest_hits;
    uint64_t shadow_rays;        /* FScene::Occluded calls (integrator.cc:367)                            */
    uint64_t shadow_occluded;
    double   render_ms;          /* device time of the last jp_render*, HIP events on the context stream  */
    double   extend_ms, shade_ms, shadow_ms, other_ms;   /* per kernel class, when profiling is enabled   */
    uint64_t extend_launches, shade_launches, shadow_launches;
    /* ABI 5: the fused schedule (k_path: ray generation and every bounce of a queue region in one launch, DESIGN.md "One schedule").
     * When it runs, extend_ms / shade_ms / shadow_ms stay 0 and path_ms is the sum of the k_path launches. */
    double   path_ms;
    uint64_t path_launches;
    /* ABI 6: reference semantics with the certified walk (JpBuildInfo.certified_walk): rays (closest-hit and shadow) whose result the
     * ordered walk could not certify and which were walked again node for node the reference's way */
    uint64_t certified_fallback_rays;
} JpCounters;

/* what jp_upload_scene did with the hierarchy */
typedef struct JpBuildInfo {
    int32_t built_on_device;     /* 1: built by the device LBVH pass, 0: the caller's tree was used          */
    int32_t traversal_mode;      /* 0 binary tree in HBM, 1 binary tree in LDS, 2 flat leaf list, 3 binary + 8-wide */
    int32_t bvh_nodes, bvh_height;
    double  device_build_ms;     /* HIP-event time of the device build (0 when the caller's tree was used)     */
    int32_t libm_sincosf;        /* which build of the host libm's sinf/cosf/sincosf the device reproduces bit for bit:
                                    1 = glibc's FMA build, 2 = its build without contraction, 0 = none (own correctly
                                    rounded evaluation; films then differ from the host reference by rare path flips)  */
    int32_t lanes_last_render;   /* stream lanes the last jp_render* used (1-4; DESIGN.md "Stream lanes")                      */
    /* ABI 5: the last jp_render* ran the fused schedule (1) or the per-bounce launches of rounds 1-2 (0: JETPBRT_FUSED=0, scenes
     * whose tables do not fit LDS, the Whitted / debug integrators); region size and resident workgroups of that launch */
    int32_t fused_last_render, fused_region, fused_workgroups;
    int32_t q4_nodes;            /* ABI 5: nodes of the 4-wide quantised tree the closest-hit rays walk (0: none; scenes of <= 1024 primitives, device-built
                                    and reference-semantics trees, JETPBRT_Q4=0) */
    int32_t libm_xbsdf;          /* ABI 5: bit 0: the device reproduces the host libm's logf / expf / powf / acosf / atanf / tanf bit for bit (the BSDF
                                    classes behind jp_bsdf that call them are then bit-exact against the reference); bit 1: with libm's FMA build */
    int32_t certified_walk;      /* ABI 6: bvh_reference_semantics on a large scene: 1 = the rays take an ordered walk over the LEAVES of the caller's tree and
                                    carry a proof that FBVH_Node::Intersect returns the same hit; the few that cannot are walked again verbatim
                                    (DESIGN.md "Certified walk"; JETPBRT_CERTIFIED=0: every ray verbatim, as in ABI <= 5) */
    int32_t certified_nodes;     /* nodes of the 4-wide tree over the caller's leaves */
    int32_t certified_eye_leaves;/* leaves of the caller's tree holding a primitive whose plane passes through the camera position (within 5e-3 of its distance):
                                    camera rays are not culled by distance there (DESIGN.md "Certified walk") */
} JpBuildInfo;


/* ABI 7: everything a host application may want to steer, by value (round 3 read 42 JETPBRT_* environment variables at upload / render time).
 * Set with jp_set_options BEFORE the jp_upload_scene / jp_render* calls it is to affect; fields left 0 keep the library's defaults (tri-state
 * switches: 0 default, 1 on, -1 off).  The environment is read ONCE, in jp_create_context, as the initial value of this struct (JETPBRT_<FIELD> in
 * capitals; "0" means off): a test override, not an interface.  jp_get_options returns the values in force. */
typedef struct JpOptions {
    int32_t struct_bytes;        /* sizeof(JpOptions) of the caller (a longer struct of a later ABI is truncated, a shorter one zero-extended) */
    /* ---- schedule (jp_render*) ---- */
    int32_t lanes;               /* stream lanes per GPU, 1-4 (0: by frame size -- three for the benchmark frames; DESIGN.md "Stream lanes")  */
    int32_t lane_rows;           /* rows per lane group (0: 4)                                                                                 */
    int32_t blocks_per_cu;       /* workgroups (= queue regions) per CU and launch (0: 16; 5 per lane with three lanes)                        */
    int64_t max_slots;           /* cap on the path slots of one batch (0: from free device memory, <= 2^26)                                   */
    int32_t compact_regions;     /* k_raygen: a region = consecutive (pixel block, sample) chunks (default for scenes walked through HBM)      */
    int32_t fused;               /* 1: the single-launch schedule k_path (DESIGN.md "One schedule"; measured slower, kept for its 1.2 GB of queues) */
    int32_t fused_region, fused_job_spp, fused_workgroups;   /* its region size / samples per job / resident workgroups per CU (0: defaults)  */
    /* ---- traversal (jp_upload_scene) ---- */
    int32_t traversal;           /* force a traversal mode for a host-built tree: 1 + mode (1: binary tree in HBM, 2: binary tree in LDS, 3: flat leaf list, 4: + 8-wide shadow tree); 0: by scene size */
    int32_t q4;                  /* closest-hit rays of large scenes through the 4-wide quantised tree (default on)                            */
    int32_t q4_shadow;           /* ... and their shadow rays (default on; off: the 8-wide tree)                                               */
    int32_t persist;             /* lane refill in the traversal kernels of large scenes: idle lanes that trigger a refill, 8 / 16 / 32 (0: 16; -1: one ray per lane) */
    int32_t vote;                /* per-iteration node / leaf vote of the refill kernels (default on, off for the verbatim reference walk)    */
    int32_t stack_lds_words;     /* traversal-stack words per thread kept in LDS, the rest spills to HBM (0: 12)                               */
    int32_t shade_sort;          /* k_shade partitions its region by material class (default: scenes with more than one material kind)         */
    int32_t device_tree;         /* hierarchy built on the device: 1 PLOC clustering (default), 2 LBVH (Karras) topology                       */
    int32_t device_wide;         /* device build: also the 8-wide shadow tree (default on)                                                     */
    int32_t bvh_max_leaf;        /* device build: primitives per leaf (0: 2 for PLOC, 3 for LBVH)                                              */
    int32_t ploc_radius, ploc_max_rounds;   /* PLOC neighbour search radius (0: 16) and round limit (0: 512; beyond it the LBVH topology serves) */
    /* ---- reference semantics, certified walk (JpScene.bvh_reference_semantics = 2; DESIGN.md "Certified walk") ---- */
    int32_t certified;           /* -1: walk every ray verbatim even when the scene asks for the certified walk (it never turns the certified walk ON for a scene that asked for the verbatim one) */
    float   cert_slack;          /* K of the distance-cull slack tmax + K eps / (mean leaf diagonal) tmax^2 for rays not from the camera (0: 16384; < 0: none) */
    float   cert_slack_eye;      /* the same for rays from the camera position (0: 1024; < 0: none)                                            */
    float   cert_eye_tau;        /* a leaf is "edge-on to the camera" when |n.(p - eye)| <= tau |p - eye| (0: 5e-3; < 0: no flags)             */
    /* ---- host libm the device reproduces (0: probe the running libm in jp_create_context) ---- */
    int32_t libm_sincosf;        /* 1 / 2: glibc's FMA / plain build; -1: none (own correctly rounded evaluation)                              */
    int32_t libm_xbsdf;          /* bit 0 exact, bit 1 FMA build; -1: none                                                                     */
    /* ---- diagnostics (tests, tools/) ---- */
    int32_t trace_walk;          /* jp_trace on a large scene walks: 0 what the render's closest-hit rays walk, 1 the binary tree, 2 the 8-wide tree, 3 the caller's tree verbatim */
    float   box_pad;             /* every box of a host-built tree grows by this many scene units (fringe census, tools/gpu_fringe_census.py)  */
    int32_t reserved[8];         /* [0] == 1: the next jp_render* uses the generic kernels (every shape, light and material alternative compiled in) even
                                    where the uploaded scene's feature set allows a lean instance -- tests and A/B runs; same films either way.  [1..7]: 0 */
} JpOptions;

typedef struct JpContext JpContext;

const char* jp_last_error(void);
int  jp_abi_version(void);
/* which build of the host libm's sinf / cosf / sincosf the device will reproduce (JpBuildInfo.libm_sincosf): probes the
 * host's libm against the library's transcription of glibc's algorithm on 200,000 arguments.  Pure host code, no GPU needed. */
int  jp_probe_libm_sincosf(void);
/* the same for logf / expf / powf / acosf / atanf / tanf (JpBuildInfo.libm_xbsdf) */
int  jp_probe_libm_xbsdf(void);

/* one context per process per GPU (device_id = LOCAL_RANK) */
int  jp_create_context(int device_id, JpContext** out);
int  jp_destroy_context(JpContext* ctx);
/* ABI 7: options by value (see JpOptions); jp_set_options(ctx, NULL) restores the defaults of jp_create_context (environment overrides included) */
int  jp_set_options(JpContext* ctx, const JpOptions* options);
int  jp_get_options(JpContext* ctx, JpOptions* out);

/* validates every index in `scene` on the host, then copies it into device-resident SoA tables */
int  jp_upload_scene(JpContext* ctx, const JpScene* scene);

/* replaces FIntegrator::Render (integrator.cc:35-80): blocking; fills film_rgb (width*height*3 floats,
 * row-major, top row first, film.h:51-57) with Clamp01(sum_s Li_s / spp) (integrator.cc:89-108).
 * Values are SET, i.e. the result of AddColor onto the zero-initialised film of film.h:30-35. */
int  jp_render(JpContext* ctx, const JpRenderParams* params, float* film_rgb_host);
/* same, film left in device memory (film_rgb_device must hold width*height*3 floats on ctx's device);
 * asynchronous on the context stream unless `sync` != 0.  Used for the multi-GPU reduce. */
int  jp_render_device(JpContext* ctx, const JpRenderParams* params, void* film_rgb_device, int sync);
/* the film output step right after the hot path (FFilm::SaveAsImage, film.cc:11-145, main.cc:160): the same render, but the
 * film leaves the device as 8-bit gamma-encoded RGB -- gamma_encoding of film.h:24, (uint8_t)(pow(Clamp01(x), 1/2.2f) * 255.0),
 * applied on the GPU after the resolve -- so a BMP / PPM writer downloads width*height*3 BYTES instead of 12 bytes per pixel.
 * rgb8_host: width*height*3 bytes, row-major, top row first, R G B.  film_rgb_host may be NULL (8-bit image only) or receive
 * the fp32 film as jp_render does.  The encoding is byte-identical to the host libm's powf: the library tabulates, once per
 * process, the 255 fp32 thresholds at which the host's gamma_encoding steps (binary search over the float bit patterns of
 * [0, 1]) and the device counts the thresholds <= x (jp_gamma_thresholds: that table, for tests). */
int  jp_render_rgb8(JpContext* ctx, const JpRenderParams* params, uint8_t* rgb8_host, float* film_rgb_host);
int  jp_gamma_thresholds(float* out255);
/* test hook (pure host code): every fp32 value of [0, 1] -- 1,065,353,217 bit patterns, n_threads host threads -- through the host's
 * gamma_encoding and through the threshold table; returns the number of values whose bytes differ (0: the device tone map is
 * byte-identical for EVERY input; the table's binary search assumes the host's powf-based curve never steps down) */
long long jp_gamma_sweep(int n_threads);
int  jp_synchronize(JpContext* ctx);
/* bytes of device memory the library holds in this process right now, over all contexts (every allocation goes through one owner type,
 * which counts it): a destroyed context gives back exactly what it took, which is what tests/test_gpu_memory.py asserts.  No GPU call. */
long long jp_device_bytes_in_use(void);

/* per-kernel-class event timing (adds two events per launch); off by default */
int  jp_set_profiling(JpContext* ctx, int enabled);
int  jp_get_counters(JpContext* ctx, JpCounters* out);
int  jp_get_build_info(JpContext* ctx, JpBuildInfo* out);

/* A BSDF of bsdf.h / bsdf.cc / microfacet.cc described by value: every class of the reference's reflection API, including the
 * ones no material instantiates (FPhongSpecularReflection bsdf.h:557-633, BeckmannDistribution microfacet.cc:11-254,
 * FMicrofacetTransmission bsdf.cc:80-145, FresnelNoOp bsdf.h:664-667). */
enum { JP_BSDF_LAMBERT = 0, JP_BSDF_MIRROR = 1, JP_BSDF_FRESNEL_SPECULAR = 2, JP_BSDF_MICROFACET_REFLECTION = 3,
       JP_BSDF_MICROFACET_TRANSMISSION = 4, JP_BSDF_PHONG = 5 };
enum { JP_DIST_TROWBRIDGE_REITZ = 0, JP_DIST_BECKMANN = 1 };
enum { JP_FRESNEL_CONDUCTOR = 0, JP_FRESNEL_DIELECTRIC = 1, JP_FRESNEL_NOOP = 2 };
typedef struct JpBsdfDesc
{
    int32_t kind;                /* JP_BSDF_*                                                                                   */
    float   color[3];            /* albedo / R / Kr / T / Ks                                                                    */
    float   color2[3];           /* FRESNEL_SPECULAR: Kt                                                                        */
    float   eta_a, eta_b;        /* FRESNEL_SPECULAR: etaI, etaT; MICROFACET_TRANSMISSION: etaA, etaB                           */
    int32_t distribution;        /* JP_DIST_*       (microfacet kinds)                                                          */
    float   alpha_x, alpha_y;    /* as handed to the distribution's constructor (clamped to >= 0.001 there)                     */
    int32_t sample_visible;      /* sampleVisibleArea (microfacet.h:33-39)                                                      */
    int32_t fresnel;             /* JP_FRESNEL_*    (MICROFACET_REFLECTION)                                                     */
    float   fr_eta_i[3], fr_eta_t[3], fr_k[3];   /* conductor: etaI, etaT, k; dielectric: fr_eta_i[0], fr_eta_t[0]              */
    float   exponent;            /* PHONG                                                                                        */
} JpBsdfDesc;
/* test hook / utility: FBSDF::Evalf, ::Pdf and ::Sample (bsdf.h:284-302) of `desc` for n shading events on the device.  Host arrays:
 * normal / wo / wi 3n floats (world space; the frame is FFrame(normal), geometry.h:345-349), u 2n floats ->
 * f_eval 3n, pdf_eval n (for wo, wi); s_f 3n, s_wi 3n, s_pdf n, s_flags n (eBSDFType bits) for Sample(wo, u). */
int  jp_bsdf(JpContext* ctx, const JpBsdfDesc* desc, int32_t n, const float* normal, const float* wo, const float* wi, const float* u,
             float* f_eval, float* pdf_eval, float* s_f, float* s_wi, float* s_pdf, int32_t* s_flags);

/* test hook: closest-hit query for n rays (FScene::Intersect, scene.cc:25-33).  Host arrays:
 * origin/dir 3n floats, tmin/tmax n floats -> hit (0/1), t (ray.max_t after the call), prim (-1 if none),
 * normal 3n floats (FIntersection::normal).  Runs the same device traversal the render uses. */
int  jp_trace(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax,
              int32_t* hit, float* t, int32_t* prim, float* normal);

/* test hook like jp_trace (additive to ABI 7): the any-hit query for n rays (FScene::Occluded), one ray per lane through the any-hit half of the device traversal
 * (what the render's shadow rays run).  Host arrays as for jp_trace -> occluded (0/1), nothing else.  It walks the structure the render's shadow rays walk;
 * JpOptions::trace_walk 1 / 2 / 3 force the binary tree, the 8-wide tree and the caller's tree verbatim exactly as for jp_trace, so both hooks can be put on
 * one structure; reserved[0] == 1 the generic tiny-scene instance.  walk_out (may be NULL): the traversal mode that ran (0 binary tree in global memory, 1 in
 * LDS, 2 flat leaf list, 3 8-wide tree, 4 4-wide tree, 5 caller's tree verbatim, 6 certified walk), + 16 for the flat-shape instance of mode 2. */
int  jp_occluded(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax,
                 int32_t* occluded, int32_t* walk_out);

/* Texture-mapped materials (additive to ABI 7; INTEGRATION.md "Textures").  A material's main colour -- MATTE diffuseColor, MIRROR specularColor,
 * PLASTIC Kd (its Qd then follows the sampled Kd at every shading point, material.h:94-98) -- may come from a texture of texture.h / texture.cc,
 * sampled on the device at every bounce of the path integrator.  Textures on GLASS / METAL are refused ([0..2] is eta there).
 *   SOLID    the colour tex_color[0..2]
 *   CHECKER  odd tex_color[0..2] where sinf(10x) * sinf(10y) * sinf(10z) < 0 at the world hit point, else even tex_color[3..5]
 *   IMAGE    nearest texel of FImageTexture::Sample: u, v clamped to [0, 1], v flipped, i = (int)(u * width), j = (int)(v * height), each
 *            clamped to size - 1 (a NaN coordinate: texel 0 on its axis); colour (1.0f / 255.0f) * byte
 * uv per shape: FRectangle::GetUV, FDisk::GetUV, FSphere::GetUV on (p - center) / radius, triangles by barycentrics of the normal equations. */
enum { JP_TEXTURE_SOLID = 0, JP_TEXTURE_CHECKER = 1, JP_TEXTURE_IMAGE = 2 };
typedef struct JpTextures {
    int32_t struct_bytes;                    /* sizeof(JpTextures) of the caller                                                    */
    int32_t n_textures;
    const int32_t *tex_type;                 /* JP_TEXTURE_*                                                                        */
    const float   *tex_color;                /* 6 per texture: SOLID [0..2]; CHECKER odd [0..2], even [3..5]                         */
    const int32_t *tex_width, *tex_height;   /* IMAGE (1 .. 16384 each)                                                             */
    const int64_t *tex_offset;               /* IMAGE: byte offset of its top-left texel in `texels`                                */
    int64_t n_texel_bytes; const uint8_t *texels;   /* RGB8, row-major, top row first, 3*width bytes per row                       */
    int32_t n_materials;   const int32_t *mat_texture;   /* == JpScene.n_materials; -1 = the material's own colour                 */
    int32_t n_triangles;   const float *tri_uv;          /* == JpScene.n_triangles; uv0 uv1 uv2 (6 floats); NULL = 0               */
} JpTextures;
typedef struct JpTextureInfo {
    int32_t struct_bytes, n_textures, n_textured_materials;
    int64_t texel_bytes_device;              /* bytes of the device's RGBA8 texel pool                                              */
    int32_t textured_last_render;            /* the last jp_render* ran k_texel + k_shade_tex                                       */
} JpTextureInfo;
/* jp_upload_scene plus the textures (validated completely on the host: JP_ERR_INVALID_ARGUMENT with a message, the context stays usable).
 * textures NULL or n_textures 0: exactly jp_upload_scene, which in turn drops the texture state of an earlier textured upload.  A textured scene
 * renders with the path integrator (the Whitted integrator returns JP_ERR_UNSUPPORTED, the debug integrator ignores textures) and the per-bounce
 * launches (JpOptions.fused falls back, fused_last_render 0). */
int  jp_upload_scene_textured(JpContext* ctx, const JpScene* scene, const JpTextures* textures);
int  jp_get_texture_info(JpContext* ctx, JpTextureInfo* out);
/* test hook / utility, like jp_trace: closest hit, then the shape's uv (2n floats) and the colour the textured slot takes there (3n floats;
 * untextured materials: mat_params[0..2]; glass, metal, no material, no hit: 0); prim: the caller's primitive index, -1 if none */
int  jp_surface(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax,
                int32_t* prim, float* uv, float* albedo);

/* Guides and denoising (additive to ABI 7; INTEGRATION.md "Guides and denoising").  A low-spp film is noisy; the first-hit feature buffers
 * ("guides": albedo, normal, depth) are not, and an edge-avoiding a-trous wavelet filter steered by them removes most of the noise.
 *
 * jp_render_guides: first-hit feature buffers of the frame `params` describes (width, height, seed, sampler_mode, band shard fields; spp,
 * max_depth and integrator are ignored).  guide_spp camera samples per pixel (1 .. 1024), sample indices 0 .. guide_spp-1 of the SAME counter
 * stream the render uses (so sample s here is the camera ray of sample s of jp_render; JP_SAMPLER_DEBUG: the pixel centre; the stock sampler:
 * JP_ERR_UNSUPPORTED as for jp_render).  The closest hit comes from the walk jp_surface uses.  Per sample:
 *              hit                                                                                        miss
 *   albedo     the colour jp_surface reports; where it reports 0 by definition (glass, metal, no         (1,1,1)
 *              material): (1,1,1)
 *   normal     FIntersection::normal as jp_trace returns it                                              (0,0,0)
 *   depth      the hit distance t                                                                        0
 * Per pixel and channel: acc = 0; for s in 0 .. guide_spp-1: acc += v_s; out = acc * (1.0f / guide_spp) -- fp32, in sample order, one thread per
 * pixel: deterministic and independent of the schedule options.  Pixels outside the band shard are 0 in all three buffers, so shards sum to the
 * full buffers like films do.  albedo 3*W*H, normal 3*W*H, depth W*H floats, row-major, top row first; any of the three may be NULL. */
int  jp_render_guides(JpContext* ctx, const JpRenderParams* params, int32_t guide_spp, float* albedo, float* normal, float* depth);
int  jp_render_guides_device(JpContext* ctx, const JpRenderParams* params, int32_t guide_spp, void* albedo_dev, void* normal_dev, void* depth_dev, int sync);

/* jp_denoise: needs no scene -- a film and guides from anywhere will do (rank 0 after a multi-GPU reduce).  All fp32, no contraction, operations
 * in the order written; only + - * / max min, so the device result is bit-identical to a restatement on any IEEE host:
 *   a = max(albedo, 0.001f) per channel if demodulating, else 1.  c0 = film / a.
 *   kn = 1/(sn*sn), kz = 1/(sz*sz), kc_i = 4^i / (sc*sc), computed in fp32 on the host.
 *   iteration i = 0 .. n-1, step s = 2^i, taps (dy, dx) in {-2..2}^2, dy outer, dx inner, tap pixel q = p + s*(dx, dy); taps outside the image are
 *   skipped.  h = {1/16, 1/4, 3/8, 1/4, 1/16}, hh = h[dy+2] * h[dx+2].
 *     dc = ((dr*dr + dg*dg) + db*db) of c_p - c_q; dn likewise of n_p - n_q; m = max(max(z_p, z_q), 1e-20f), rz = (z_p - z_q) / m, dz = rz*rz
 *     w = hh / (((1 + dc*kc_i) * (1 + dn*kn)) * (1 + dz*kz));  num += w * c_q (per channel), den += w
 *   c_next_p = num / den;  out = Clamp01(c_n * a) -- or max(c_n * a, 0) while the context's film state has hdr = 1 (jp_set_film, "Film" below: the
 *   parameters do not grow; the context decides, for jp_denoise* and jp_render_denoised alike).
 * Defaults (fields left 0): iterations 5, sigma_color 1.0, sigma_normal 0.1, sigma_depth 0.03, demodulation on (DESIGN.md "Denoiser": the grid
 * they were chosen from).  film / albedo / normal / depth / out laid out as jp_render and jp_render_guides lay them out; albedo may be NULL only
 * with demodulate = -1; out may not overlap an input (JP_ERR_INVALID_ARGUMENT).  Working buffers belong to the context and are reused. */
typedef struct JpDenoiseParams {
    int32_t struct_bytes, width, height;
    int32_t iterations;                                  /* 1..6; 0: 5                                                       */
    float   sigma_color, sigma_normal, sigma_depth;      /* > 0 and finite; 0: the library's default                         */
    int32_t demodulate;                                  /* 0 default (on), 1 on, -1 off                                     */
} JpDenoiseParams;
int  jp_denoise(JpContext* ctx, const JpDenoiseParams* params, const float* film_rgb, const float* albedo, const float* normal, const float* depth, float* out_rgb);
int  jp_denoise_device(JpContext* ctx, const JpDenoiseParams* params, const void* film_dev, const void* albedo_dev, const void* normal_dev, const void* depth_dev, void* out_dev, int sync);
/* jp_render, jp_render_guides, jp_denoise (params NULL: guides only, the film as rendered; its width / height are taken from `render`) and, with
 * rgb8_host, the tone map of jp_render_rgb8 on the result, in one call: the film stays on the device between the stages.  film_host or rgb8_host
 * may be NULL (not both); albedo / normal / depth may be NULL.  The bytes are those of the separate calls. */
int  jp_render_denoised(JpContext* ctx, const JpRenderParams* render, int32_t guide_spp, const JpDenoiseParams* params, float* film_host, uint8_t* rgb8_host,
                        float* albedo, float* normal, float* depth);
/* what the last jp_render_guides* / jp_denoise* of the context did (HIP-event times on the context stream, kernels only; synchronises the stream) */
typedef struct JpDenoiseInfo {
    int32_t struct_bytes, iterations;                    /* iterations of the last jp_denoise*                                */
    float   sigma_color, sigma_normal, sigma_depth;      /* the values in force in it                                         */
    int32_t demodulated, guide_spp;
    double  denoise_ms, guides_ms;
} JpDenoiseInfo;
int  jp_get_denoise_info(JpContext* ctx, JpDenoiseInfo* out);

/* Light selection (additive to ABI 7; INTEGRATION.md "Light selection").  JP_LIGHTS_ALL: the reference's estimator, every light sampled at every
 * non-delta bounce (at most 255 lights).  JP_LIGHTS_POWER_ONE: one light per bounce, picked with probability proportional to its power from an alias
 * table, its contribution divided by that probability: one shadow ray and one shadow plane per bounce for up to 2^24 lights (emissive meshes).
 *   weight (double, from the fp32 scene values, s = (double)r + g + b):  AREA (s * area) * pi, area = the fp32 FShape::Area() of the upload;
 *     POINT s * (4 * pi);  DIRECTION, ENVIRONMENT (s * pi) * ((double)world_radius * world_radius).  W = the weights summed in light order;
 *     pmf_i = (float)(w_i / W), all 0 when W == 0 (then no light is sampled).
 *   table: Vose's alias method in double; bin i holds the fp32 threshold q[i] and alias[i]; a light of weight 0 is in no bin's reach.
 *   pick from two draws: i = min((int)(u0 * (float)n), n - 1);  j = u1 < q[i] ? i : alias[i].
 *   a non-delta bounce draws: [the plastic closure draw], u0, u1, the two draws of FLight::Sample_Li for light j (consumed even when the sample is
 *     rejected), then the BSDF sample.  Contribution: (cmul(cmul(beta, f), Li) * absdot / pdf) / pmf_j.
 * Path integrator only (Whitted: JP_ERR_UNSUPPORTED; the debug integrator ignores the mode); JpOptions.fused falls back to the per-bounce launches. */
enum { JP_LIGHTS_ALL = 0, JP_LIGHTS_POWER_ONE = 1 };
typedef struct JpLightSampling { int32_t struct_bytes; int32_t mode; } JpLightSampling;
/* takes effect with the next jp_upload_scene*; NULL: back to JP_LIGHTS_ALL */
int  jp_set_light_sampling(JpContext* ctx, const JpLightSampling* sampling);
typedef struct JpLightInfo {
    int32_t struct_bytes, mode, n_lights;    /* mode and light count of the uploaded scene                                   */
    int32_t n_selectable;                    /* lights of weight > 0 (POWER_ONE; ALL: the non-black lights)                   */
    double  total_weight;                    /* W (0 in ALL mode)                                                            */
    int32_t picked_last_render;              /* the last jp_render* ran the pick kernels (k_shade_pick / k_shade_pick_tex)   */
} JpLightInfo;
int  jp_get_light_info(JpContext* ctx, JpLightInfo* out);
/* the table in force, downloaded from the device: n_lights entries each (any pointer may be NULL); JP_ERR_UNSUPPORTED for a scene uploaded in ALL mode */
int  jp_get_light_table(JpContext* ctx, float* q, int32_t* alias, float* pmf);
/* test hook like jp_trace: the device's selection (the function the render calls) for n pairs of draws -> index (-1 for a scene without lights), pmf */
int  jp_light_pick(JpContext* ctx, int32_t n, const float* u0, const float* u1, int32_t* index, float* pmf);
/* the table builder of the upload; pure host code, no GPU needed.  weights: n finite values >= 0 (else JP_ERR_INVALID_ARGUMENT); n == 0 is JP_OK */
int  jp_build_light_table(int32_t n, const double* weight, float* q, int32_t* alias, float* pmf);

/* Environment maps (additive to ABI 7; INTEGRATION.md "Environment maps" has the definition).  A lat-long fp32 RGB image, width x height texels, row-major,
 * top row first, 1 <= width, height <= 4096, every value finite and >= 0.  Row r covers the polar angle [pi r / H, pi (r + 1) / H] from the map's up axis,
 * column c the azimuth [2 pi c / W, 2 pi (c + 1) / W].  JP_ENV_UP_Z: map space is world space (the reference's SphericalTheta / SphericalPhi);
 * JP_ENV_UP_Y: map (x, y, z) = world (z, x, y).  The map is context state like the light sampling mode: the next jp_upload_scene* reads it.  That scene
 * must hold exactly one JP_LIGHT_ENVIRONMENT light (else JP_ERR_INVALID_ARGUMENT), whose light_radiance tints the map (device texel = tint * texel in fp32),
 * and be uploaded with JP_LIGHTS_POWER_ONE (else JP_ERR_UNSUPPORTED): the map light is one entry of the light table, weight (mean_sum * pi) * R^2.
 * A miss at bounce 0 or after a specular bounce adds beta * the nearest texel; when the light table returns the map light, five draws a0 a1 a2 b0 b1
 * follow u0 u1 in place of the light's two: the texel from an alias table over the texels (weight: (r + g + b) * solid angle of the row's texels;
 * importance = -1: the solid angle alone), then a place inside it uniform in (cos theta, phi).  Path integrator only (Whitted: JP_ERR_UNSUPPORTED; the
 * debug integrator and jp_render_guides ignore the map); JpOptions.fused falls back to the per-bounce launches. */
enum { JP_ENV_UP_Z = 0, JP_ENV_UP_Y = 1 };
typedef struct JpEnvMap {
    int32_t struct_bytes;                    /* sizeof(JpEnvMap)                                                              */
    int32_t width, height, up_axis;          /* up_axis: JP_ENV_UP_*                                                          */
    int32_t importance;                      /* 0: sample by radiance x solid angle; -1: by solid angle alone (A/B, tests)    */
    const float* rgb;                        /* 3 * width * height values; copied by jp_set_environment_map                   */
} JpEnvMap;
/* validates and copies the map; takes effect with the next jp_upload_scene*; NULL: no map */
int  jp_set_environment_map(JpContext* ctx, const JpEnvMap* map);
typedef struct JpEnvInfo {
    int32_t struct_bytes, width, height, up_axis, importance;   /* the uploaded scene's map (all 0: none)                     */
    int32_t n_selectable;                    /* texels of weight > 0                                                          */
    double  total_weight;                    /* W_env: the texel weights summed in row-major order                            */
    double  mean_sum;                        /* sum over texels of (r + g + b) * solid angle / (4 pi): the map light's "radiance sum" */
    int32_t mapped_last_render;              /* the last jp_render* ran the map kernels (k_shade_env / k_shade_env_tex)       */
    int64_t table_bytes_device;              /* device bytes of the texel, bin and row tables                                 */
} JpEnvInfo;
int  jp_get_env_info(JpContext* ctx, JpEnvInfo* out);
/* test hooks like jp_trace: the device functions the render calls.  lookup: n directions (3 floats each, world space, finite) -> texel index, tinted rgb.
 * sample: n times five draws in [0, 1) (a0 a1 a2 b0 b1) -> texel index, world-space wi, Li, pdf.  Any output pointer may be NULL.
 * JP_ERR_UNSUPPORTED for a scene uploaded without a map. */
int  jp_env_lookup(JpContext* ctx, int32_t n, const float* dir, int32_t* texel_index, float* rgb);
int  jp_env_sample(JpContext* ctx, int32_t n, const float* u, int32_t* texel_index, float* wi, float* Li, float* pdf);
/* the table builder of the upload; pure host code, no GPU needed.  tint: 3 floats (NULL: 1 1 1).  Outputs (any may be NULL): weight, q, alias: W * H each;
 * texel: 4 floats per texel (tinted r g b, pdf); row_cos: 2 floats per row; total: W_env; mean_sum: as JpEnvInfo. */
int  jp_build_environment_table(const JpEnvMap* map, const float* tint, double* weight, float* q, int32_t* alias, float* texel, float* row_cos, double* total, double* mean_sum);

/* Estimator (additive to ABI 7; INTEGRATION.md "Estimator" has the definition).  JP_ESTIMATOR_NEE: the reference's -- emission counts on bounce 0 and after
 * a specular bounce, next-event estimation does the rest.  JP_ESTIMATOR_MIS: at a non-delta shading event both ways of reaching an emitter count -- the
 * direction drawn on the picked light and the direction the BSDF sample takes -- each weighted with the power heuristic (exponent 2) of the two pdfs, so a
 * glossy surface under a large emitter, or a matte one just below it, no longer hangs on the strategy that samples it badly.  The draws, their order and
 * every ray are those of JP_LIGHTS_POWER_ONE: the same paths with other weights, the same JpCounters ray counts, and the same film wherever every weight
 * is 1 (delta lights, specular chains).  Render-time state: takes effect with the next jp_render*, so one upload serves both.  Needs a scene uploaded with
 * JP_LIGHTS_POWER_ONE (else JP_ERR_UNSUPPORTED from jp_render*, the context stays usable), with or without a map, textured or not.  Path integrator only
 * (Whitted: JP_ERR_UNSUPPORTED; the debug integrator and jp_render_guides ignore it); JpOptions.fused falls back to the per-bounce launches. */
enum { JP_ESTIMATOR_NEE = 0, JP_ESTIMATOR_MIS = 1 };
typedef struct JpEstimator { int32_t struct_bytes; int32_t mode; } JpEstimator;
/* NULL: back to JP_ESTIMATOR_NEE; an unknown mode: JP_ERR_INVALID_ARGUMENT */
int  jp_set_estimator(JpContext* ctx, const JpEstimator* estimator);
typedef struct JpEstimatorInfo {
    int32_t struct_bytes, mode;              /* the mode in force                                                              */
    int32_t mis_last_render;                 /* the last jp_render* ran the MIS kernels (k_shade_mis*)                          */
    int64_t side_bytes_device;               /* device bytes of the per-path side records (0 until the first MIS render)        */
} JpEstimatorInfo;
int  jp_get_estimator_info(JpContext* ctx, JpEstimatorInfo* out);
/* test hook like jp_trace: n rays (unit directions) through the walk jp_trace uses -> the light reached (the emitter primitive's light where it emits toward
 * the origin; on a miss the map light, else the first non-black constant environment light; -1: none) and the light strategy's solid-angle pdf at the origin
 * for it, pmf * pdf_Li -- 0 where that light cannot be sampled from there (delta lights, the interior of a sphere light, a pdf that is not finite or not
 * positive).  JP_ERR_UNSUPPORTED for a scene uploaded with JP_LIGHTS_ALL. */
int  jp_light_pdf(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* light, float* pdf);

/* Vertex normals (additive to ABI 7; INTEGRATION.md "Vertex normals" has the definition).  tri_vn: 9 floats per triangle of JpScene's triangle arrays, the unit
 * normals n0 n1 n2 at p0 p1 p2.  Nine zeros mark the triangle flat (shaded with tri_n, as without normals); otherwise every value must be finite and each
 * normal satisfy 0.81 <= |n|^2 <= 1.21 (else JP_ERR_INVALID_ARGUMENT with a message, the context stays usable).  Context state like the map and the light mode:
 * validated and copied here, read by the next jp_upload_scene* (whose n_triangles must equal this one's, else JP_ERR_INVALID_ARGUMENT); NULL removes them.
 * At a hit on a smooth triangle the path integrator builds the BSDF frame, wo and both cosine factors from the interpolated normal Ns (include/jp_normals.h)
 * and keeps tri_n for everything that belongs to the surface as an emitter or as geometry; a sampled direction on the other geometric side than wo is refused
 * (matte, mirror, plastic, metal).  All eight combinations of light sampling x map x estimator, textured or not.  Whitted: JP_ERR_UNSUPPORTED for a scene with
 * at least one smooth triangle; the debug integrator ignores the normals; JpOptions.fused falls back to the per-bounce launches; jp_render_guides delivers Ns
 * in its normal buffer.  Normals that are all flat: exactly the upload without normals (smooth_last_render 0, bit-identical films and guides). */
typedef struct JpVertexNormals { int32_t struct_bytes; int32_t n_triangles; const float* tri_vn; } JpVertexNormals;
int  jp_set_vertex_normals(JpContext* ctx, const JpVertexNormals* normals);
typedef struct JpNormalInfo {
    int32_t struct_bytes, n_triangles, n_smooth_triangles;   /* of the uploaded scene's normals (0 0: uploaded without)                          */
    int64_t table_bytes_device;              /* device bytes of the 48-byte-per-primitive normal table (0: no smooth triangle)              */
    int32_t smooth_last_render;              /* the last jp_render* ran k_normal and the smooth kernels (k_shade_smooth*)                    */
    double  normal_ms;                       /* with jp_set_profiling: k_normal's launches of the last render (a share of JpCounters.shade_ms) */
} JpNormalInfo;
int  jp_get_normal_info(JpContext* ctx, JpNormalInfo* out);
/* test hook like jp_surface: the walk jp_trace takes, then prim (the caller's primitive index, -1 on a miss), Ng as jp_trace returns its normal and the Ns the
 * render uses there (3n floats each; Ns == Ng on flat triangles and other shapes; both 0 on a miss) */
int  jp_shading_normal(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* prim, float* ng, float* ns);
/* the very function the device runs (include/jp_normals.h), for n points: p0 p1 p2 ng p 3 floats each, vn9 9 floats each -> ns_out 3 floats each.  Pure host
 * code, no GPU needed; so is jp_check_vertex_normals, the validation of jp_set_vertex_normals with its status and message (n_smooth may be NULL). */
int  jp_interpolate_normals(int32_t n, const float* p0, const float* p1, const float* p2, const float* ng, const float* vn9, const float* p, float* ns_out);
int  jp_check_vertex_normals(const JpVertexNormals* normals, int32_t* n_smooth);

/* Normal maps (additive to ABI 7; INTEGRATION.md "Normal maps" has the definition, include/jp_normal_map.h the code).  A material may carry a tangent-space
 * normal map: RGB8 texels (row-major, top row first) decoded as max((b - 128) / 127, -1), looked up bilinearly between texel centres with clamp addressing at the
 * uv of the hit (tri_uv here for triangles -- the struct's own set, independent of JpTextures.tri_uv; GetUV of the other shapes), x and y multiplied by the
 * material's strength, and turned into the shading normal Ns' in the frame (T, B, Nb) of the base normal Nb -- Ns of a smooth triangle, else the geometric
 * normal.  Context state like the vertex normals: validated and copied here (JP_ERR_INVALID_ARGUMENT with a message, the context keeps what it had), read by the
 * next jp_upload_scene*, whose n_materials and n_triangles must equal these; NULL removes them.  Ns' takes Ns's place everywhere (jp_set_vertex_normals above):
 * every material kind, all combinations of light sampling x map x estimator, textured or not; Whitted: JP_ERR_UNSUPPORTED; the debug integrator ignores the
 * maps; JpOptions.fused falls back; jp_shading_normal and the normal guide deliver Ns'.  No mapped material, strength 0 or maps whose R and G are 128
 * everywhere: exactly the upload without maps (mapped_last_render 0, bit-identical films and guides). */
typedef struct JpNormalMaps {
    int32_t struct_bytes;
    int32_t n_maps;        const int32_t *map_width, *map_height;   /* 1 .. 16384 each */
    const int64_t *map_offset;  int64_t n_texel_bytes;  const uint8_t *texels;   /* RGB8, row-major, top row first */
    int32_t n_materials;   const int32_t *mat_map;      /* == JpScene.n_materials; -1: none */
    const float *mat_strength;                          /* per material, finite; NULL: 1 for all */
    int32_t n_triangles;   const float *tri_uv;         /* == JpScene.n_triangles; uv0 uv1 uv2; NULL: 0 (triangles then stay unperturbed) */
} JpNormalMaps;
int  jp_set_normal_maps(JpContext* ctx, const JpNormalMaps* maps);          /* NULL removes them */
int  jp_check_normal_maps(const JpNormalMaps* maps, int32_t* n_mapped_materials);   /* pure host: the same validation, status and message; materials with mat_map >= 0 (may be NULL) */
typedef struct JpNormalMapInfo {
    int32_t struct_bytes, n_maps, n_mapped_materials;   /* of the uploaded scene's maps (0 0: uploaded without)                                  */
    int64_t texel_bytes_device, table_bytes_device;     /* the texel pool (one dword per texel); descriptors, material and uv records (0: nothing perturbs) */
    int32_t mapped_last_render;                         /* the last jp_render* ran k_normal_map                                                 */
    double  normal_map_ms;                              /* with jp_set_profiling: k_normal_map's launches of the last render (a share of JpCounters.shade_ms) */
} JpNormalMapInfo;
int  jp_get_normal_map_info(JpContext* ctx, JpNormalMapInfo* out);
/* pure host, the very function the device runs, for n points: nb, ng, dpdu, dpdv 3 floats each, uv 2 floats, one map (w, h, rgb8), strength -> ns_out 3 floats
 * (nb where unperturbed), perturbed_out 0/1 */
int  jp_perturb_normals(int32_t n, const float* nb, const float* ng, const float* dpdu, const float* dpdv, const float* uv,
                        int32_t width, int32_t height, const uint8_t* rgb8, float strength, float* ns_out, int32_t* perturbed_out);
/* pure host: dpdu, dpdv of a triangle from its corners and uvs as the header defines them; ok_out 0 (and both 0) where det is 0 or not finite */
int  jp_triangle_tangents(int32_t n, const float* p0, const float* p1, const float* p2, const float* uv6, float* dpdu, float* dpdv, int32_t* ok_out);

/* Texture sampling (additive to ABI 7; INTEGRATION.md "Texture sampling" has the definition, include/jp_tex_sampling.h the code).  A record per image texture and
 * per normal map: a wrap mode per axis, a uv scale and offset (t = c * scale + offset) and a filter.  Bilinear colour lookups are quantised to 8 bits per channel
 * (the side word of the nearest lookup).  Normal maps take CLAMP or REPEAT and their bilinear filter; scales are > 0.  Context state like the normal maps: validated
 * and copied here, read by the next jp_upload_scene*, whose JpTextures.n_textures must equal n_textures where tex != NULL (a plain jp_upload_scene counts as 0) and
 * whose JpNormalMaps.n_maps must equal n_maps where map != NULL (no maps set: 0): else JP_ERR_INVALID_ARGUMENT, and the context keeps the scene it had.  A record
 * that is not the identity on a SOLID or CHECKER texture is refused at the upload.  No state, or identity records only (CLAMP, the kind's filter, scale 1,
 * offset 0): exactly the upload without them -- the same kernels, sampled_last_render 0, no device bytes.  Else k_texel_s / k_normal_map_s take the place of
 * k_texel / k_normal_map, and jp_surface, jp_shading_normal and the guides follow the records. */
enum { JP_WRAP_CLAMP = 0, JP_WRAP_REPEAT = 1, JP_WRAP_MIRROR = 2 };
enum { JP_FILTER_DEFAULT = 0, JP_FILTER_NEAREST = 1, JP_FILTER_BILINEAR = 2 };   /* DEFAULT: nearest for colour textures, bilinear for normal maps */
typedef struct JpTexSampler { int32_t wrap_u, wrap_v, filter; float scale_u, scale_v, offset_u, offset_v; } JpTexSampler;
typedef struct JpTextureSampling {
    int32_t struct_bytes;
    int32_t n_textures;  const JpTexSampler* tex;      /* one per texture of the next upload's JpTextures; NULL: none for colour textures */
    int32_t n_maps;      const JpTexSampler* map;      /* one per map of jp_set_normal_maps;              NULL: none for normal maps     */
} JpTextureSampling;
typedef struct JpTexSamplingInfo {
    int32_t struct_bytes, n_active_textures, n_active_maps;   /* records of the uploaded scene that are not the identity                            */
    int64_t table_bytes_device;                               /* 32 bytes per texture and per map (0: nothing active)                                */
    int32_t sampled_last_render;                              /* the last jp_render* ran k_texel_s or k_normal_map_s                                 */
    double  texel_ms, normal_map_ms;                          /* with jp_set_profiling: the launches of k_texel / k_texel_s and of k_normal_map / k_normal_map_s of the last render */
} JpTexSamplingInfo;
int  jp_set_texture_sampling(JpContext* ctx, const JpTextureSampling* sampling);   /* NULL removes it */
int  jp_check_texture_sampling(const JpTextureSampling* sampling, int32_t* n_active_textures, int32_t* n_active_maps);   /* pure host: the same validation, status and message (counts may be NULL) */
int  jp_get_texture_sampling_info(JpContext* ctx, JpTexSamplingInfo* out);
/* pure host, the very function the device runs: n uv pairs on one image (w, h, rgb8 row-major, top row first) -> rgb8_out 3 bytes each; the colour is (1 / 255) * byte.
 * NULL or an identity record: the lookup without records */
int  jp_texture_lookup(const JpTexSampler* s_or_null, int32_t w, int32_t h, const uint8_t* rgb8, int32_t n, const float* uv, uint8_t* rgb8_out);
/* pure host: jp_perturb_normals with the map addressed through a record (NULL or identity: jp_perturb_normals) */
int  jp_perturb_normals_sampled(const JpTexSampler* s_or_null, int32_t n, const float* nb, const float* ng, const float* dpdu, const float* dpdv, const float* uv,
                                int32_t width, int32_t height, const uint8_t* rgb8, float strength, float* ns_out, int32_t* perturbed_out);

/* Mip maps (additive to ABI 7; INTEGRATION.md "Mip maps" has the definition, include/jp_mipmap.h the code).  A mode per image texture: with JP_MIP_TRILINEAR the
 * upload builds the texture's pyramid on the device (box filter, integers) behind the texel pool, and the path integrator carries a ray cone per path slot
 * (width, spread: 8 bytes) from which the side kernel k_texel_m -- in k_texel / k_texel_s's place -- takes the footprint rho of every textured hit in texels and
 * filters trilinearly between levels floor(log2 rho) and the next.  rho <= 1 is exactly the lookup without mipmaps.  footprint_scale multiplies rho (0: 1);
 * bounce_spread (radians; 0: 0.125, a design choice) is the least spread of the cone after a bounce that is not specular.  Context state like the sampling
 * records: validated and copied here, read by the next jp_upload_scene*, whose JpTextures.n_textures must equal n_textures (a plain jp_upload_scene counts as 0):
 * else JP_ERR_INVALID_ARGUMENT, and the context keeps the scene it had.  JP_MIP_TRILINEAR on a SOLID or CHECKER texture is refused at the upload.  No state, all
 * modes OFF, or mipmaps only on textures no material uses: exactly the upload without them -- the same kernels, mip_last_render 0, no device bytes.  The guides'
 * albedo follows the mip at the first hit (width = gamma0 * t); jp_surface has no cone and reads level 0.  Normal maps are not mip-mapped. */
enum { JP_MIP_OFF = 0, JP_MIP_TRILINEAR = 1 };
typedef struct JpTextureMipmaps { int32_t struct_bytes, n_textures; const int32_t* mode; float footprint_scale, bounce_spread; } JpTextureMipmaps;   /* mode NULL: all OFF */
typedef struct JpTextureMipmapInfo {
    int32_t struct_bytes, n_on;                       /* textures of the uploaded scene whose pyramid was built (mode TRILINEAR, used by a material)          */
    int32_t n_levels;                                 /* their levels in all, level 0 included                                                               */
    int32_t mip_last_render;                          /* the last jp_render* ran k_texel_m                                                                   */
    int64_t pyramid_bytes_device;                     /* levels >= 1, 4 bytes per texel, plus the level tables                                               */
    int64_t cone_bytes_device;                        /* 8 bytes per path slot, over all lanes (0 until a render needs it)                                   */
    double  build_ms;                                 /* the k_mip_level launches of the upload (HIP events)                                                 */
    double  texel_ms;                                 /* with jp_set_profiling: the side kernel's launches of the last render (JpTexSamplingInfo.texel_ms)  */
    float   footprint_scale, bounce_spread, gamma0;   /* the values in force (defaults resolved); gamma0 = 2 |cam.up| / res_y of the uploaded camera         */
} JpTextureMipmapInfo;
int  jp_set_texture_mipmaps(JpContext* ctx, const JpTextureMipmaps* mipmaps);      /* read by the next upload; NULL removes */
int  jp_check_texture_mipmaps(const JpTextureMipmaps* mipmaps, int32_t* n_on);     /* pure host: the same validation, status and message (n_on may be NULL) */
int  jp_get_texture_mipmap_info(JpContext* ctx, JpTextureMipmapInfo* out);
/* the uploaded pyramid of one texture, copied from the device: levels in order, 3 bytes per texel; capacity in bytes (JP_ERR_INVALID_ARGUMENT when too small or
 * the texture has no pyramid) */
int  jp_read_mip_chain(JpContext* ctx, int32_t texture, uint8_t* rgb8_out, int64_t capacity);
/* pure host: the pyramid of a w x h image, levels in order into rgb8_out (3 bytes per texel; level 0 is the image); level_w / level_h: 15 entries at least.
 * rgb8_out NULL: only the sizes */
int  jp_build_mip_chain(int32_t w, int32_t h, const uint8_t* rgb8, uint8_t* rgb8_out, int32_t* level_w, int32_t* level_h, int32_t* n_levels);
/* pure host: one hit for each of n independent cones: state_inout[2k .. 2k+1] = (width, spread) of cone k before the hit at distance t[k] of a ray with the
 * flags word flags[k] (bounce in bits 0-7, bit 8: the ray left a specular closure), overwritten with the state after it; a path is a chain of calls */
int  jp_mip_cone_step(float gamma0, float bounce_spread, int32_t n, const int32_t* flags, const float* t, float* state_inout /*2n*/);
/* pure host: rho of n hits from the cone's width and the world area per unit uv area A at the hit (include/jp_mipmap.h has A per shape) */
int  jp_mip_footprint(int32_t n, const float* width, const float* area, int32_t w, int32_t h, float scale_u, float scale_v, float footprint_scale, float* rho_out);
/* pure host: jp_texture_lookup at a footprint of rho texels per lookup, on the image's pyramid */
int  jp_texture_lookup_mip(const JpTexSampler* s_or_null, int32_t w, int32_t h, const uint8_t* rgb8, int32_t n, const float* uv, const float* rho, uint8_t* rgb8_out);
/* test hook like jp_surface: the closest hit of the same walk, then the very device function k_texel_m calls on the caller's flags and (width, spread) state:
 * state_inout 2 floats per ray, updated as at a hit; prim -1 (state untouched, rho 0, colour 0) on a miss; rho 0 and the bytes of the lookup without mipmaps where the
 * hit's image has no pyramid; colour 0 for an untextured hit and for a SOLID or CHECKER texture (their side word is no texel).  Needs a scene uploaded with at least
 * one pyramid */
int  jp_mip_probe(JpContext* ctx, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, const int32_t* flags, float* state_inout,
                  int32_t* prim, float* rho, uint8_t* rgb8);

/* Procedural textures (additive to ABI 7; INTEGRATION.md "Procedural textures" has the definition, include/jp_procedural.h the code).  A record per texture
 * turns a JP_TEXTURE_CHECKER texture into gradient noise, fBm, turbulence, marble or the box-filtered checker between the texture's two colours
 * (c_even = tex_color[3..5] at t = 0, c_odd = tex_color[0..2] at t = 1; both in [0, 1]: the result is an RGB8 side word).  The lookup point is q = M x + t with
 * x the hit point (SPACE_WORLD) or (u, v, 0) (SPACE_UV) and m the row-major 3 x 4 map.  With antialias on (the default) the side kernel k_texel_p -- in
 * k_texel / k_texel_s / k_texel_m's place -- band-limits the texture by the footprint of the path's ray cone (the cone of the mip maps: 8 bytes per path
 * slot): octaves whose wavelength falls below the footprint fade out and the loop over them ends early.  Context state like the mipmap modes: validated and
 * copied here, read by the next jp_upload_scene*, whose JpTextures.n_textures must equal n_textures.  The rules that need the textures (a record on a texture
 * that is not CHECKER, colours outside [0, 1], SPACE_UV without tri_uv) are checked at the upload: JP_ERR_INVALID_ARGUMENT, and the context keeps the scene it
 * had.  No state, all kinds NONE, or records only on textures no material uses: exactly the upload without them -- the same kernels, procedural_last_render 0,
 * no device bytes.  The guides' albedo follows the procedural colour at the first hit (width = gamma0 * t). */
enum { JP_PROC_NONE = 0, JP_PROC_NOISE = 1, JP_PROC_FBM = 2, JP_PROC_TURBULENCE = 3, JP_PROC_MARBLE = 4, JP_PROC_CHECKER_AA = 5 };
enum { JP_PROC_SPACE_WORLD = 0, JP_PROC_SPACE_UV = 1 };
typedef struct JpProcedural {
    int32_t kind, space;                              /* JP_PROC_*, JP_PROC_SPACE_*                                                                          */
    float   m[12];                                    /* row-major 3 x 4: q = M x + t; finite, linear part not singular                                      */
    int32_t octaves;                                  /* 1 .. 12; 0: 6 (NOISE has one octave whatever this says)                                             */
    float   gain;                                     /* amplitude ratio between octaves, (0, 1]; 0: 0.5                                                     */
    float   variation;                                /* MARBLE: the weight of the fBm in the stripe coordinate; 0: 1                                        */
    int32_t antialias;                                /* 0: default (on), 1: on, -1: off                                                                     */
} JpProcedural;
typedef struct JpTextureProcedurals { int32_t struct_bytes, n_textures; const JpProcedural* rec; } JpTextureProcedurals;   /* rec NULL: all NONE */
typedef struct JpProceduralInfo {
    int32_t struct_bytes, n_procedural;               /* textures of the uploaded scene with a record (kind not NONE, used by a material)                    */
    int32_t n_antialiased;                            /* ... of them with antialias on                                                                       */
    int32_t procedural_last_render;                   /* the last jp_render* ran k_texel_p                                                                   */
    int64_t table_bytes_device;                       /* the records and the per-texture index                                                               */
} JpProceduralInfo;
int  jp_set_texture_procedurals(JpContext* ctx, const JpTextureProcedurals* procedurals);   /* read by the next upload; NULL removes */
/* pure host: the same validation, status and message; textures_or_null: also the rules of the upload against these textures (n_textures must match).
 * n_procedural counts the records that are not NONE, n_antialiased those of them with antialias on (either may be NULL) */
int  jp_check_texture_procedurals(const JpTextureProcedurals* procedurals, const JpTextures* textures_or_null, int32_t* n_procedural, int32_t* n_antialiased);
int  jp_get_procedural_info(JpContext* ctx, JpProceduralInfo* out);
/* pure host: the lookup of one record (kind not NONE) as texture index `texture` at n points: p 3n floats, uv 2n, width n (the cone's width at the hit; 0: no
 * cone) -> word_out n side words (the colour's RGB8 under the image tag, or the plain checker's colour index 2 * texture + parity under the colour tag) and
 * t_out n blend parameters (either may be NULL) */
int  jp_procedural_lookup(const JpProcedural* rec, const float* c_even, const float* c_odd, int32_t texture, int32_t n, const float* p, const float* uv, const float* width,
                          uint32_t* word_out, float* t_out);
/* test hook: the device twin of jp_procedural_lookup on the uploaded record and colours of texture `texture` (kernel k_proc_probe, no traversal) */
int  jp_procedural_probe(JpContext* ctx, int32_t texture, int32_t n, const float* p, const float* uv, const float* width, uint32_t* word_out);

/* Lens (additive to ABI 7; INTEGRATION.md "Lens" has the definition).  The reference's camera is a pinhole: every camera ray starts at JpCamera.pos.  A lens of
 * radius > 0 gives depth of field: the camera ray of a sample starts at a point of the aperture -- a disk (blades 0) or a regular polygon of 3 .. 16 blades with
 * circumradius `radius`, its first vertex rotation_deg from the camera's right axis toward its up axis -- and passes through the point where the pinhole ray meets
 * the plane of focus, the set pos + focus_distance * d0 with d0 = front + right * a + up * b the pinhole's direction before normalisation (a plane at depth
 * focus_distance * |front| along front when right and up are perpendicular to front).  Rays are weighted uniformly, like the pinhole's.  Draws: dims 0, 1 the
 * film position as ever, dims 2, 3 the lens, the path's first bounce starts at dim 4 (without a lens: 2).  JP_SAMPLER_DEBUG draws (0.5, 0.5): the centre of the
 * disk -- the pinhole's rays from origin pos -- and for a polygon the point the formula gives: the centre again for an even number of blades (w = 0), and
 * v[(n-1)/2] * b + v[(n+1)/2] * b with b = 0.5f * sqrtf(0.5f) for an odd one, a point on the axis of the middle blade, not the centre.  Render-time state like the estimator: read by the next jp_render* /
 * jp_render_guides* (sample s of the guides stays the camera ray of sample s of the render), so one upload serves every lens; NULL or radius 0: the pinhole,
 * the kernels and films of a context that never heard of a lens.  Every integrator, every combination of the additive features; JpOptions.fused falls back to the
 * per-bounce launches.  Reference semantics 1 and 2 are allowed: lens rays do not start at the camera position, so the certified walk treats them like
 * secondary rays (the wider distance-cull slack, the verbatim walk behind it).  The lens owns no device memory. */
typedef struct JpLens { int32_t struct_bytes; float radius, focus_distance; int32_t blades; float rotation_deg; } JpLens;
/* validates (jp_check_lens: JP_ERR_INVALID_ARGUMENT with a message, the lens in force stays): radius finite and >= 0; focus_distance finite and > 0 whenever
 * radius > 0; blades 0 or 3 .. 16; rotation_deg finite */
int  jp_set_lens(JpContext* ctx, const JpLens* lens);
typedef struct JpLensInfo { int32_t struct_bytes; float radius, focus_distance; int32_t blades; float rotation_deg; int32_t lens_last_render; } JpLensInfo;   /* the lens in force (all 0: the pinhole); the last jp_render* ran k_raygen<true> / the lens branch of k_other */
int  jp_get_lens_info(JpContext* ctx, JpLensInfo* out);
/* pure host code, no GPU needed: the validation of jp_set_lens with its status and message */
int  jp_check_lens(const JpLens* lens);
/* pure host code: the JpLensPlan (include/jp_lens.h) the kernels receive by value for `lens` on `camera`.  plan_out NULL: *bytes receives its size and nothing is
 * copied; capacity smaller than the plan: JP_ERR_INVALID_ARGUMENT.  lens NULL or radius 0: JP_OK and 0 bytes (no plan: the pinhole). */
int  jp_lens_plan(const JpCamera* camera, const JpLens* lens, void* plan_out, int64_t capacity, int64_t* bytes);
/* pure host code: the very function the device runs (include/jp_lens.h) for n samples: fxfy 2n floats (the film position: pixel + draws 0, 1), u 2n floats (draws
 * 2, 3) -> origin, dir 3n floats each.  lens NULL or radius 0: the pinhole's rays (u may then be NULL). */
int  jp_lens_rays(const JpCamera* camera, const JpLens* lens, int32_t n, const float* fxfy, const float* u, float* origin, float* dir);
/* test hook like jp_trace: what k_raygen forms for sample s[i] of pixel (x[i], y[i]) (0 <= x < width, 0 <= y < height, s >= 0) under params' seed and sampler_mode
 * (width and height bound x and y; its other fields are not read) and the lens in force, on the uploaded scene's camera: origin, dir 3n floats each, dim_next n values -- the dimension the path's
 * first bounce draws from (4 with a lens, 2 without).  Any output pointer may be NULL. */
int  jp_camera_rays(JpContext* ctx, const JpRenderParams* params, int32_t n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin, float* dir, int32_t* dim_next);
/* autofocus: the pinhole ray through the film position (fx, fy) (pixels, fractional) of the uploaded scene's camera, along the walk jp_trace takes (tmin 0.001, no
 * far end): *focus_out = t / |d0|, the focus_distance that puts the hit on the plane of focus; a miss: JP_OK and 0 */
int  jp_focus_distance(JpContext* ctx, float fx, float fy, float* focus_out);

/* Projections (additive to ABI 7; INTEGRATION.md "Projections" has the definitions).  The reference's camera is the perspective pinhole.  A projection replaces
 * how the camera ray of a film position is formed -- nothing else: same draws (dims 0, 1; the path's first bounce starts at dim 2), same queue records, same bounces.
 * With a = fx / res_x - 0.5, b = 0.5 - fy / res_y and the unit axes ex, ey, ez of right, up, front:
 *   JP_PROJ_ORTHOGRAPHIC  origin pos + right * (a * s) + up * (b * s), direction ez (s = ortho_scale; 0 means 1): the rectangle the pinhole's film spans at
 *                         parameter distance s, whatever the depth
 *   JP_PROJ_EQUIRECT      origin pos, direction ez * (cos theta * cos phi) + ex * (cos theta * sin phi) + ey * sin theta, phi = 2 pi a, theta = pi b: a lat-long
 *                         panorama -- the centre looks along front, the top row toward up, column 0 directly behind
 *   JP_PROJ_FISHEYE       origin pos, equidistant: x = fx - res_x / 2, y = res_y / 2 - fy, rho = |(x, y)|, theta = min(rho / R * fov / 2, pi), direction
 *                         ez * cos theta + (ex * x + ey * y) * (sin theta / rho); R the half-diagonal, half-width or half-height in pixels (fit); fov_deg in
 *                         (0, 360], 0 means 180.  Every pixel has a ray
 * Render-time state like the lens: read by the next jp_render* / jp_render_guides* / jp_camera_rays; NULL or kind 0: the pinhole, the kernels and films of a context
 * that never heard of a projection.  Every integrator; JpOptions.fused falls back to the per-bounce launches; a lens (radius > 0) together with a projection is
 * refused by the render (JP_ERR_UNSUPPORTED).  Equirect and fisheye need perpendicular camera axes (pairwise |dot| of the unit axes <= 1e-3), checked at render
 * time on the uploaded camera.  The ray cone of a camera ray starts with the projection's spread (equirect pi / res_y, fisheye (fov / 2) / R, orthographic 0: a
 * first hit reads the finest mip level).  jp_focus_distance stays the pinhole's.  A projection owns no device memory. */
enum { JP_PROJ_PERSPECTIVE = 0, JP_PROJ_ORTHOGRAPHIC = 1, JP_PROJ_EQUIRECT = 2, JP_PROJ_FISHEYE = 3 };
enum { JP_FIT_DIAGONAL = 0, JP_FIT_WIDTH = 1, JP_FIT_HEIGHT = 2 };
typedef struct JpProjection { int32_t struct_bytes, kind; float ortho_scale, fov_deg; int32_t fit; } JpProjection;
/* validates (jp_check_projection: JP_ERR_INVALID_ARGUMENT with a message, the projection in force stays): kind 0 .. 3; ortho_scale finite and >= 0; fov_deg finite
 * in [0, 360]; fit 0 .. 2 */
int  jp_set_projection(JpContext* ctx, const JpProjection* projection);
/* the projection in force (all 0: the pinhole); the last jp_render* ran k_raygen_proj / the projected branch of k_other, and the cone spread it used (0 when it
 * did not) */
typedef struct JpProjectionInfo { int32_t struct_bytes, kind; float ortho_scale, fov_deg; int32_t fit, projected_last_render; float gamma0_last_render; } JpProjectionInfo;
int  jp_get_projection_info(JpContext* ctx, JpProjectionInfo* out);
/* pure host code, no GPU needed: the validation of jp_set_projection with its status and message */
int  jp_check_projection(const JpProjection* projection);
/* pure host code: the JpProjectionPlan (include/jp_projection.h) the kernels receive by value for `projection` on `camera`, with the checks the render makes on the
 * camera.  plan_out NULL: *bytes receives its size and nothing is copied.  projection NULL or kind 0: JP_OK and 0 bytes (no plan: the pinhole). */
int  jp_projection_plan(const JpCamera* camera, const JpProjection* projection, void* plan_out, int64_t capacity, int64_t* bytes);
/* pure host code: the very function the device runs (include/jp_projection.h) for n film positions fxfy (2n floats: pixel + draws 0, 1) -> origin, dir 3n floats
 * each.  projection NULL or kind 0: the pinhole's rays. */
int  jp_projection_rays(const JpCamera* camera, const JpProjection* projection, int32_t n, const float* fxfy, float* origin, float* dir);

/* Film (additive to ABI 7; INTEGRATION.md "Film" has the definitions in full).  The reference's film holds Clamp01(sum / spp); that stays the default.  The film state
 * below adds the linear-light film: unclamped output, a per-sample firefly clamp, a luminance histogram for auto-exposure and a display transform.  All of it is
 * fp32, operation by operation, no contraction (include/jp_film.h, include/jp_tonemap.h: the text the kernels and the pure-host entry points both compile), so
 * device and host agree bit for bit.  With no film state and no tone map set, every kernel, film, guide and byte is what it is without this section.
 *
 * jp_set_film: render-time state like the lens (read by the next jp_render*; one upload serves every film state; lanes and the fused schedule take it too).
 *   hdr 1: the last batch of the per-pixel sum writes max(L, 0) per channel instead of Clamp01(L); the sum itself -- L += l * (1.0f / spp) in sample order, across
 *     batches -- is the same, so clip(film_hdr, 0, 1) is the default film bit for bit.
 *   sample_clamp c > 0 (finite; 0: off): each sample's radiance l is replaced before it enters the sum: any channel not finite -> (0, 0, 0); else with
 *     m = max(max(l.r, l.g), l.b): m > c -> l * (c / m) (one division, three multiplications); else l.  Works with hdr 0 or 1.
 *   NULL, or {hdr 0, sample_clamp 0}: the reference's film, the kernels of a context that never heard of a film state; hdr_last_render is then 0.
 *   Every integrator; band shards as ever (pixels outside the shard are 0, shards sum to the full film).
 * While the film state in force has hdr = 1, jp_denoise* and jp_render_denoised end with max(c_n * a, 0) instead of Clamp01(c_n * a) (JpDenoiseParams does not grow). */
typedef struct JpFilm { int32_t struct_bytes; int32_t hdr; float sample_clamp; } JpFilm;
int  jp_set_film(JpContext* ctx, const JpFilm* film);          /* NULL: the reference's film */
int  jp_check_film(const JpFilm* film);                        /* pure host: the validation of jp_set_film, same status and message */
typedef struct JpFilmInfo { int32_t struct_bytes, hdr; float sample_clamp; int32_t hdr_last_render; } JpFilmInfo;   /* the state in force; hdr_last_render: the last jp_render* ran the film instance of k_resolve */
int  jp_get_film_info(JpContext* ctx, JpFilmInfo* out);
/* pure host, the very function the device runs on each sample: n rgb triples in -> out (may alias).  film NULL or sample_clamp 0: a copy */
int  jp_film_samples(const JpFilm* film, int32_t n, const float* in_rgb, float* out_rgb);

/* Luminance histogram of a tightly packed rgb film (needs no scene).  Per pixel Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b; !(Y > 0) or Y not finite: counted in
 * hist[JP_FILM_BINS] (excluded); else k = (int)(bits(Y) >> 21) - 380 -- four bins per octave, split by the top two mantissa bits, k = 0 at 2^-32 -- and the bin is
 * min(max(k, 0), 255).  Integer counts: independent of the order, equal to a restatement on any host.  hist: JP_FILM_BINS + 1 dwords (the device variant zeroes
 * them on the stream first).  The working buffer belongs to the context and is reused. */
#define JP_FILM_BINS 256
int  jp_film_histogram(JpContext* ctx, int32_t width, int32_t height, const float* film_rgb, uint32_t* hist);
int  jp_film_histogram_device(JpContext* ctx, int32_t width, int32_t height, const void* film_dev, void* hist_dev, int sync);

/* Display transform: exposure, a tone curve, then the byte-exact gamma table of jp_render_rgb8.
 *   defaults (fields left 0): key 0.18, white 4.0, pct_low 0.05, pct_high 0.95.  Validation: every field finite, key and white > 0, 0 <= pct_low < pct_high <= 1,
 *   a known curve and mode.
 *   exposure scale (host, double): MANUAL scale = (float)exp2((double)ev).  AUTO: over bins 0 .. 255 with N their total, c_k = the part of bin k's span of the
 *   cumulative count that lies inside [pct_low * N, pct_high * N] (bins straddling an end count fractionally); centre_k = (1.125 + 0.25 * (k & 3)) * 2^((k >> 2) - 32);
 *   Lavg = exp2(sum(c_k * log2(centre_k)) / sum(c_k)); scale = (float)(key / Lavg * exp2(ev)); N == 0 or sum(c_k) == 0: scale 1.
 *   per value: t = x * scale; v = t > 0 ? min(t, 1e9f) : 0 (NaN and negatives: 0);
 *     CLAMP    y = v
 *     REINHARD y = (v * (1 + v / (white*white))) / (1 + v)
 *     ACES     y = (v * (2.51f*v + 0.03f)) / (v * (2.43f*v + 0.59f) + 0.14f)                                  (Narkowicz's fit)
 *     HABLE    y = h(2*v) / h(11.2f),  h(x) = ((x*(0.15f*x + 0.05f) + 0.004f) / (x*(0.15f*x + 0.5f) + 0.06f)) - 0.02f/0.3f
 *   y = Clamp01(y): rgb_out receives y, rgb8_out the number of thresholds of jp_gamma_thresholds that are <= y.  CLAMP, MANUAL, ev 0: jp_render_rgb8's bytes.
 * jp_set_tonemap: render-time state; while one is in force jp_render_rgb8 and jp_render_denoised produce their bytes with it (AUTO: histogram on the device, 257
 * dwords read back, the scale on the host, then the transform) and mapped_last_render is 1; NULL: none, k_tonemap8 as ever.  The tone map applies to whatever
 * film the film state produced: a curve other than CLAMP wants hdr = 1 (highlights above 1 are what the curves compress). */
enum { JP_CURVE_CLAMP = 0, JP_CURVE_REINHARD = 1, JP_CURVE_ACES = 2, JP_CURVE_HABLE = 3 };
enum { JP_EXPOSURE_MANUAL = 0, JP_EXPOSURE_AUTO = 1 };
typedef struct JpToneMap { int32_t struct_bytes, curve, exposure_mode; float ev, key, white, pct_low, pct_high; } JpToneMap;
int  jp_set_tonemap(JpContext* ctx, const JpToneMap* tonemap);
int  jp_check_tonemap(const JpToneMap* tonemap);               /* pure host: the validation, same status and message; NULL: JP_OK */
int  jp_exposure_from_histogram(const JpToneMap* tonemap, const uint32_t* hist, float* scale_out);   /* pure host; MANUAL: hist may be NULL */
/* tonemap NULL: the one in force (none in force: JP_ERR_INVALID_ARGUMENT).  w * h pixels of a tightly packed rgb film -> rgb8_out (3 bytes per pixel) and / or
 * rgb_out (3 floats per pixel): either may be NULL, not both.  scale_out (may be NULL): the exposure scale used.  Needs no scene.  The device variant with AUTO
 * synchronises the stream to read the histogram back. */
int  jp_tonemap(JpContext* ctx, const JpToneMap* tonemap, int32_t width, int32_t height, const float* film_rgb, uint8_t* rgb8_out, float* rgb_out, float* scale_out);
int  jp_tonemap_device(JpContext* ctx, const JpToneMap* tonemap, int32_t width, int32_t height, const void* film_dev, void* rgb8_dev, void* rgb_dev, float* scale_out, int sync);
/* pure host, the very function the device runs: n_values floats -> bytes and / or floats under `scale` */
int  jp_tonemap_host(const JpToneMap* tonemap, float scale, int64_t n_values, const float* in, uint8_t* rgb8_out, float* rgb_out);
typedef struct JpToneMapInfo { int32_t struct_bytes, curve, exposure_mode; float scale_last; int32_t mapped_last_render; double histogram_ms, tonemap_ms; } JpToneMapInfo;
int  jp_get_tonemap_info(JpContext* ctx, JpToneMapInfo* out);  /* curve / mode in force (0 0: none); scale and kernel times of the last transform; synchronises the stream */

/* ---- Variance (additive to ABI 7; INTEGRATION.md "Variance") --------------------------------------------------------------------------------------
 * A render that also delivers the per-pixel variance of its own mean, and a variance-guided variant of the a-trous filter.  All of it is fp32, operation by
 * operation, no contraction (include/jp_variance.h: the text the kernels and jp_variance_samples both compile).  With none of these calls made, every kernel,
 * film, guide and byte is what it is without this section.
 *
 * The estimate.  Per pixel, over its samples in sample-index order k = 1 .. spp, with l the sample's radiance as it enters the film's sum (after the sample clamp
 * of jp_set_film where one is in force):
 *     y = (0.2126f*l.r + 0.7152f*l.g) + 0.0722f*l.b                       (y not finite -> 0)
 *     d = y - mean;  mean = mean + d / (float)k;  m2 = m2 + d * (y - mean)           (mean = m2 = 0 before k = 1)
 *     variance = (m2 / (float)(spp - 1)) / (float)spp                     (the variance of the pixel's mean luminance)
 *   jp_render_variance*: jp_render* with that plane next to the film (W*H floats, the film's pixel layout; pixels outside the band shard are 0, so shards sum to
 *   the full plane).  The film is jp_render's bit for bit under the same state; every schedule, lane count and integrator.  spp < 2: JP_ERR_INVALID_ARGUMENT.
 *   (mean, m2) live in 8 bytes per pixel on the device while the call runs (a call with sync = 0: until the next jp_render*).  A jp_render after it runs the
 *   kernels it always ran; variance_last_render is then 0. */
int  jp_render_variance(JpContext* ctx, const JpRenderParams* params, float* film_rgb_host, float* variance_host);          /* either may be NULL, not both */
int  jp_render_variance_device(JpContext* ctx, const JpRenderParams* params, void* film_dev, void* variance_dev, int sync);
/* pure host, the very function the device runs: samples_rgb [spp][n_pixels][3]; film NULL or sample_clamp 0: no clamp; variance_out / mean_out: n_pixels floats, either may be NULL */
int  jp_variance_samples(const JpFilm* film_or_null, int32_t spp, int64_t n_pixels, const float* samples_rgb, float* variance_out, float* mean_out);
/* test hook: the device twin of jp_variance_samples on caller-supplied samples, split into batches of batch_spp (>= 1) so the carried state is exercised; needs no scene */
int  jp_variance_probe(JpContext* ctx, const JpFilm* film_or_null, int32_t spp, int32_t batch_spp, int64_t n_pixels, const float* samples_rgb, float* variance_out);
/* The variance-guided filter: jp_denoise's inputs, taps, guides, validation and no-overlap rule (extended to the two new buffers), with the colour edge-stop scaled
 * per pixel by a locally filtered variance that is carried through the iterations.  Only + - * / max min, in the order written:
 *   set-up   a = max(albedo, 0.001f) per channel (1 without demodulation); c0 = film / a; aY = (0.2126f*a.r + 0.7152f*a.g) + 0.0722f*a.b;
 *            vin = v > 0 ? min(v, 1e30f) : 0 (NaN and negatives: 0); v0 = vin / (aY*aY); kn, kz as in jp_denoise; sc2 = sigma_color*sigma_color
 *   iteration i = 0 .. n-1, step 2^i:
 *            g_p = (sum k3*v_q) / (sum k3) over q = p + (dx, dy), dx, dy in -1 .. 1 (distance 1 whatever the step; dy outer, dx inner; taps outside the image
 *                  skipped in both sums), k3 = {1/4, 1/2, 1/4}[dy+1] * {1/4, 1/2, 1/4}[dx+1]
 *            kc_p = 1.0f / (sc2 * g_p + 1e-8f)                              (no 4^i factor: the propagated variance does that job)
 *            the 25 taps of jp_denoise, dc, dn, dz, hh unchanged: w = hh / (((1 + dc*kc_p) * (1 + dn*kn)) * (1 + dz*kz));
 *                  num += w*c_q; den += w; vnum += (w*w)*v_q;   c_next_p = num / den;  v_next_p = vnum / (den*den)
 *   output   out = Clamp01(c_n * a) (max(c_n * a, 0) while the film state has hdr = 1); variance_out = v_n * (aY*aY) (may be NULL)
 * Defaults (fields left 0): as jp_denoise, but sigma_color 8.0 (DESIGN.md "Variance": the grid). */
int  jp_denoise_variance(JpContext* ctx, const JpDenoiseParams* params, const float* film_rgb, const float* albedo, const float* normal, const float* depth,
                         const float* variance, float* out_rgb, float* variance_out);
int  jp_denoise_variance_device(JpContext* ctx, const JpDenoiseParams* params, const void* film_dev, const void* albedo_dev, const void* normal_dev, const void* depth_dev,
                                const void* variance_dev, void* out_dev, void* variance_out_dev, int sync);
/* as jp_render_denoised, with jp_render_variance and jp_denoise_variance as its stages; `variance` (may be NULL) receives the render's variance plane */
int  jp_render_denoised_variance(JpContext* ctx, const JpRenderParams* render, int32_t guide_spp, const JpDenoiseParams* params, float* film_host, uint8_t* rgb8_host,
                                 float* albedo, float* normal, float* depth, float* variance);
/* variance_last_render: the last jp_render* kept the moments; moment_bytes_device: what they took (all lanes); the rest: the last jp_denoise_variance* (kernel time
 * from HIP events on the context stream; synchronises the stream) */
typedef struct JpVarianceInfo { int32_t struct_bytes, variance_last_render; int64_t moment_bytes_device; int32_t iterations; float sigma_color, sigma_normal, sigma_depth; int32_t demodulated; double denoise_ms; } JpVarianceInfo;
int  jp_get_variance_info(JpContext* ctx, JpVarianceInfo* out);

/* ---- Adaptive sampling (additive to ABI 7; INTEGRATION.md "Adaptive sampling") ------------------------------------------------------------------------
 * A render that stops each pixel by the variance of its own mean.  The rule is include/jp_adaptive.h, the text the kernels and jp_adaptive_samples both
 * compile: every pixel of the band shard takes min_spp samples; then a pixel passes when
 *     (m2 / (float)(n - 1)) / (float)n <= t * t,   t = threshold * max(mean, floor)   ((mean, m2): the moments of "Variance"; not finite on either side: pass)
 * and stays active iff it was active and does not pass (dilate 1: iff a pixel of its 3 x 3 neighbourhood, clipped to the image and the band shard, does not
 * pass); active pixels take min(step_spp, max_spp - n) more samples, the next sample indices of the stream jp_render draws, until none is active or n == max_spp.
 *     film = Clamp01(sum / (float)n) (max(., 0) while the film state has hdr = 1); counts = n (int32, 0 outside the shard); variance = (m2 / (float)(n - 1)) / (float)n
 * struct_bytes = sizeof(JpAdaptive); max_spp 0: JpRenderParams.spp; floor 0: 1e-3.  threshold 0 stops only pixels whose samples so far were all equal; min_spp = max_spp is the uniform render.
 * The path integrator on the per-bounce launches of one lane (JpOptions::fused falls back; Whitted / debug: JP_ERR_UNSUPPORTED, the context stays usable).
 * With none of these calls made every other entry point launches exactly what it launched before. */
typedef struct JpAdaptive { int32_t struct_bytes; int32_t min_spp, step_spp, max_spp; float threshold, floor; int32_t dilate; } JpAdaptive;
int  jp_check_adaptive(const JpAdaptive* adaptive);            /* pure host: the validation of jp_render_adaptive, same status and message */
/* film_rgb_host: W*H*3 floats, counts_host: W*H int32, variance_host: W*H floats; any two may be NULL */
int  jp_render_adaptive(JpContext* ctx, const JpRenderParams* params, const JpAdaptive* adaptive, float* film_rgb_host, int32_t* counts_host, float* variance_host);
/* device pointers, any two may be NULL.  The call reads the active count once per pass, so it has waited for all but its last pass whatever `sync` says; it
 * waits for the last one too before it frees the per-pixel state, which lives for the length of the call only. */
int  jp_render_adaptive_device(JpContext* ctx, const JpRenderParams* params, const JpAdaptive* adaptive, void* film_dev, void* counts_dev, void* variance_dev, int sync);
/* pure host, the very functions the device runs: the whole loop on caller-supplied samples_rgb [max_spp][height*width][3] (max_spp > 0 here); film NULL: no clamp, hdr 0 */
int  jp_adaptive_samples(const JpFilm* film_or_null, const JpAdaptive* adaptive, int32_t width, int32_t height, const float* samples_rgb, float* film_rgb, int32_t* counts, float* variance);
/* test hook: the device's k_resolve_list, k_adapt_select and k_adapt_finish on caller-supplied samples; needs no scene */
int  jp_adaptive_probe(JpContext* ctx, const JpFilm* film_or_null, const JpAdaptive* adaptive, int32_t width, int32_t height, const float* samples_rgb, float* film_rgb, int32_t* counts, float* variance);
/* the last jp_render_adaptive* / jp_adaptive_probe (adaptive_last_render 0 once a film render of another kind -- jp_render*, jp_render_rgb8, jp_render_variance*, jp_render_denoised* -- has run since: the rest then is 0; guides, filters and tone maps leave it): passes run (the first, uniform one
 * included), samples traced, the active count after each of the first 16 tests (-1: no such test), the bytes of the per-pixel state while the call ran, and
 * with jp_set_profiling the kernel time of the selection (k_adapt_select, its scan and compaction) and of k_resolve_list.  Synchronises the stream. */
typedef struct JpAdaptiveInfo { int32_t struct_bytes, adaptive_last_render, passes, min_spp, step_spp, max_spp, dilate; float threshold; int64_t samples_traced, state_bytes_device;
                                int32_t active_after[16]; double select_ms, resolve_ms; } JpAdaptiveInfo;
int  jp_get_adaptive_info(JpContext* ctx, JpAdaptiveInfo* out);

/* What jp_upload_scene would do with `scene` (additive to ABI 7; INTEGRATION.md "Describing an upload"): the scalars of the plan every later launch
 * reads, and for each table the host builds the byte count and the 64-bit FNV-1a of exactly the bytes the upload copies to the device.  Pure host code, no GPU
 * needed: the same validation (same status codes and jp_last_error texts), table builders and plan function the upload runs, nothing decided twice.
 * options NULL: the defaults (no environment); light_mode: JP_LIGHTS_*.  A scene without a hierarchy (n_bvh_nodes == 0) gets its trees from the device
 * builders: JP_ERR_UNSUPPORTED.  Set struct_bytes to sizeof(JpUploadInfo); a shorter struct is truncated. */
#define JP_UPLOAD_TABLES 11
typedef struct JpUploadTable { int64_t bytes; uint64_t fnv1a; } JpUploadTable;   /* both 0: the upload has no such table */
typedef struct JpUploadInfo {
    int32_t struct_bytes;
    int32_t trav_mode;                       /* JpBuildInfo.traversal_mode; 5: reference semantics                              */
    int32_t stack_depth, stack_depth_q4;     /* traversal stack entries of the binary / 8-wide / verbatim walks, of the 4-wide walks */
    int64_t lds_bytes, lds_bytes_shadow, shade_lds_bytes;   /* dynamic LDS of k_extend, k_shadow, k_shade                          */
    int32_t scene_in_lds, tables_in_lds, shade_prims_in_lds, stage_nee, n_planes;
    int32_t persist, vote, shade_sort, use_q4, q4_shadow, cert;
    int32_t class_mask, shape_mask, light_mask, light_shape_mask;   /* the feature set (DESIGN.md "Feature sets")                     */
    int32_t has_null_material, stack_lds_words;
    int32_t n_nodes, n_prims, n_flat, n_wide, n_q4;          /* entries of the binary tree, records, flat leaf list, 8-wide and 4-wide trees */
    int32_t bvh_nodes, bvh_height;           /* as JpBuildInfo reports them                                                     */
    int32_t wide_height, q4_height, cert_eye_leaves, n_env;
    float   cert_pad, cert_pad_eye, env_sum[3];
    JpUploadTable table[JP_UPLOAD_TABLES];   /* nodes, prims, meta, mats, mat_type, lights, shade_tab, wide, q4, refbox, flat   */
} JpUploadInfo;
int  jp_describe_upload(const JpOptions* options_or_null, int32_t light_mode, const JpScene* scene, JpUploadInfo* out);

/* Reading the tables back (additive to ABI 7; INTEGRATION.md "Reading the tables back"): test hooks, read-only.  `which` is an index into
 * JpUploadInfo.table (JP_TABLE_*).  out NULL: *bytes receives the table's size and nothing is copied; a table the upload does not have: 0 bytes, JP_OK;
 * capacity_bytes smaller than the table: JP_ERR_INVALID_ARGUMENT, nothing copied.
 * jp_copy_upload_table: pure host code, no GPU needed -- the options, validation, builders of jp_describe_upload, then the bytes whose count and FNV-1a
 *   that function reports for table `which` (any of the eleven).  JP_ERR_UNSUPPORTED for a scene without a hierarchy, as there.
 * jp_read_scene_table: the same table of the scene the context holds, copied from the device, host-built or device-built alike; the hierarchy tables only
 *   (nodes, prims, meta, wide, q4, flat; anything else: JP_ERR_INVALID_ARGUMENT).  Blocking.
 * jp_get_tree_info: the entry counts and heights that belong to those tables, as the upload's plan holds them (JpBuildInfo has no room for the wide heights). */
enum { JP_TABLE_NODES = 0, JP_TABLE_PRIMS = 1, JP_TABLE_META = 2, JP_TABLE_WIDE = 7, JP_TABLE_Q4 = 8, JP_TABLE_FLAT = 10 };
typedef struct JpTreeInfo {
    int32_t struct_bytes;                    /* sizeof(JpTreeInfo) of the caller; a shorter struct is truncated                     */
    int32_t n_prims, n_nodes, bvh_height;    /* primitive records; slots of the binary node table; emitted interior nodes on the longest root-to-leaf path */
    int32_t n_wide, wide_height;             /* 8-wide tree: nodes, levels (0 0: none)                                              */
    int32_t n_q4, q4_height;                 /* 4-wide tree: nodes, levels (0 0: none)                                              */
    int32_t n_flat;                          /* entries of the flat leaf list                                                       */
} JpTreeInfo;
int  jp_copy_upload_table(const JpOptions* options_or_null, int32_t light_mode, const JpScene* scene, int32_t which, void* out, int64_t capacity_bytes, int64_t* bytes);
int  jp_read_scene_table(JpContext* ctx, int32_t which, void* out, int64_t capacity_bytes, int64_t* bytes);
int  jp_get_tree_info(JpContext* ctx, JpTreeInfo* out);

#ifdef __cplusplus
}
#endif
#endif
