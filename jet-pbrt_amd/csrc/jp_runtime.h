// jet-pbrt_amd/csrc/jp_runtime.h -- host runtime, part 1 of 3: the context behind the C ABI (include/jetpbrt_amd.h), its ScenePlan and the device memory it owns
// (SceneTables, QueueBufs and single DevBufs of jp_devmem.h: the context's destructor is what frees them), the options (JpOptions, ABI 7), the probes of the host
// libm the device reproduces, the gamma-threshold table, jp_create_context / jp_destroy_context / jp_set_options.
// Included by jp_kernels.hip (one translation unit: the kernels above, then this host code that launches them).
#pragma once

// =====================================================================================================================
// host side: context, scene upload, render loop, C ABI
// =====================================================================================================================
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(JP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

// tri-state switch of JpOptions: 0 default, 1 on, -1 off
static inline bool opt_flag(int v, bool dflt) { return v == 0 ? dflt : v > 0; }

// The environment as the initial value of the options (read ONCE per context, in jp_create_context): a test override, not an interface.
// kind 0: integer as it is; 1: switch ("0" = off -> -1, anything else on); 2: number where "0" means none (-> -1); 3: 64-bit integer;
// 4: the device tree by name ("lbvh" -> 2, anything else PLOC); 5: presence selects the value in `as`; 6: traversal mode (stored as 1 + mode)
static void options_from_environment(JpOptions& o)
{
	struct Item { const char* name; int kind; void* field; int as; };
	const Item items[] = {
		{ "JETPBRT_LANES", 0, &o.lanes, 0 }, { "JETPBRT_LANE_ROWS", 0, &o.lane_rows, 0 }, { "JETPBRT_BLOCKS_PER_CU", 0, &o.blocks_per_cu, 0 }, { "JETPBRT_MAX_SLOTS", 3, &o.max_slots, 0 },
		{ "JETPBRT_COMPACT_REGIONS", 1, &o.compact_regions, 0 }, { "JETPBRT_FUSED", 1, &o.fused, 0 }, { "JETPBRT_REGION", 0, &o.fused_region, 0 }, { "JETPBRT_JOB_SPP", 0, &o.fused_job_spp, 0 },
		{ "JETPBRT_FUSED_WGS", 0, &o.fused_workgroups, 0 }, { "JETPBRT_TRAVERSAL", 6, &o.traversal, 0 }, { "JETPBRT_Q4", 1, &o.q4, 0 }, { "JETPBRT_Q4_SHADOW", 1, &o.q4_shadow, 0 },
		{ "JETPBRT_PERSIST", 2, &o.persist, 0 }, { "JETPBRT_VOTE", 1, &o.vote, 0 }, { "JETPBRT_STACK_LDS", 0, &o.stack_lds_words, 0 }, { "JETPBRT_SHADE_SORT", 1, &o.shade_sort, 0 },
		{ "JETPBRT_DEVICE_TREE", 4, &o.device_tree, 0 }, { "JETPBRT_DEVICE_WIDE", 1, &o.device_wide, 0 }, { "JETPBRT_BVH_MAXLEAF", 0, &o.bvh_max_leaf, 0 },
		{ "JETPBRT_PLOC_RADIUS", 0, &o.ploc_radius, 0 }, { "JETPBRT_PLOC_MAX_ROUNDS", 0, &o.ploc_max_rounds, 0 }, { "JETPBRT_CERTIFIED", 1, &o.certified, 0 },
		{ "JETPBRT_CERT_SLACK", 7, &o.cert_slack, 0 }, { "JETPBRT_CERT_SLACK_EYE", 7, &o.cert_slack_eye, 0 }, { "JETPBRT_CERT_EYE", 7, &o.cert_eye_tau, 0 },
		{ "JETPBRT_SINCOSF", 2, &o.libm_sincosf, 0 }, { "JETPBRT_LIBM", 2, &o.libm_xbsdf, 0 },
		{ "JETPBRT_TRACE_BINARY", 5, &o.trace_walk, 1 }, { "JETPBRT_TRACE_WIDE", 5, &o.trace_walk, 2 }, { "JETPBRT_TRACE_VERBATIM", 5, &o.trace_walk, 3 }, { "JETPBRT_BOX_PAD", 7, &o.box_pad, 0 },
	};
	for (const Item& it : items)
	{
		const char* e = getenv(it.name);
		if (!e || !*e) continue;
		switch (it.kind)
		{
			case 0: *(int32_t*)it.field = atoi(e); break;
			case 1: *(int32_t*)it.field = atoi(e) != 0 ? 1 : -1; break;
			case 2: { const int v = atoi(e); *(int32_t*)it.field = v != 0 ? v : -1; break; }
			case 3: *(int64_t*)it.field = atoll(e); break;
			case 4: *(int32_t*)it.field = std::string(e) == "lbvh" ? 2 : 1; break;
			case 5: *(int32_t*)it.field = it.as; break;
			case 6: { const int v = atoi(e); if (v >= 0 && v <= 3) *(int32_t*)it.field = 1 + v; break; }
			case 7: { const float v = (float)atof(e); *(float*)it.field = v != 0.f ? v : -1.f; break; }
		}
	}
}

// Everything jp_upload_scene* derives from the scene and the options that later launches read: the ONE thing a lane context takes from its
// parent (sync_lane_scene: one assignment), and the only input of the kernel selectors of jp_render.h besides the render's region size.
struct ScenePlan
{
	bool have_scene = false;
	SceneView sv; TexView tv = {}; bool textured = false;
	PickView pv = {}; bool pick = false;                                               // JP_LIGHTS_POWER_ONE (jp_pick.h): the alias table; one shadow plane, no light records in k_shade's LDS tables
	NormView nv = {}; bool smooth = false;                                             // vertex normals (jp_normals.h): at least one smooth triangle; k_shade's row is then <false, false, false>
	NMapView mp = {}; bool mapped = false;                                             // normal maps (jp_normal_map.h): at least one material whose map perturbs; smooth is then set too (the smooth row, k_normal_map in k_normal's place)
	int nm_maps = 0, nm_mapped = 0; long long nm_texel_bytes = 0, nm_table_bytes = 0;   // ... and what jp_get_normal_map_info reports of the uploaded scene's maps
	SampView sm = {}; int ts_active_textures = 0, ts_active_maps = 0; long long ts_table_bytes = 0;   // texture sampling records (jp_tex_sampling.h): the slots of the textures / maps where one is active (k_texel_s / k_normal_map_s then), and what jp_get_texture_sampling_info reports
	MipView mv = {}; int mip_on = 0, mip_levels = 0; long long mip_bytes = 0;           // mip maps (jp_mipmap.h): the level tables where a pyramid was built (k_texel_m then; mv.cone is set per launch), and what jp_get_texture_mipmap_info reports
	ProcView proc = {}; int proc_on = 0, proc_aa = 0; long long proc_bytes = 0;        // procedural textures (jp_procedural.h): the records and the per-texture index where a used texture has one (k_texel_p then), how many of them are antialiased (the cone array then), and what jp_get_procedural_info reports
	EnvView ev = {}; bool env = false; double env_mean_sum = 0.0;                      // environment map (jp_env.h): the texel tables; the map light's weight in the light table is (env_mean_sum * pi) * R^2
	int trav_mode = 0, stack_depth = 1, stack_depth_q4 = 0; bool scene_in_lds = false, shade_prims_in_lds = false; size_t lds_bytes = 0, lds_bytes_shadow = 0;
	bool cert = false;                                                                 // reference semantics, certified walk (Walker<6>)
	bool use_q4 = false, q4_shadow = false;                                            // closest-hit (and, as an experiment, shadow) rays walk the 4-wide quantised tree (Walker<4>)
	bool vote = false; int persist = 0;                                             // lane refill in the closest-hit traversal of large scenes (k_extend_persist): refill threshold, 0 = off
	int n_planes = 1; bool has_null_material = false;
	bool tables_in_lds = false, stage_nee = false; size_t shade_lds_bytes = 0;
	int class_mask = 0x3f; bool shade_sort = false;                                     // k_shade partitions its tiles by material class (scenes with more than one material kind)
	int shape_mask = 0xf, light_mask = 0xf, light_shape_mask = 0xf;                    // feature set: JP_SHAPE_* of the primitives, JP_LIGHT_* of the non-black lights, JP_SHAPE_* under the non-black area lights (bit = 1 << value); materials: class_mask
	// lane refill kernels: traversal-stack words per thread kept in LDS, the rest spills to global memory (WalkStack).  Measured on the
	// 280k-triangle scene (tree height 24): 8 / 12 / 16 words 1922 / 1926 / 1922 Msamples/s, 20 words or the whole stack 1634 / 1692.
	int stack_lds_words = 12;
};

// The device tables of an uploaded scene, owned by the context that uploaded them; the views of the plan (sv, tv, pv) point into them.
// A lane context's stay empty: it reads its parent's through the plan.
struct SceneTables
{
	DevBuf nodes, prims, meta, mats, mat_type, lights, shade_tab, flat, wide, q4, refbox;
	DevBuf tex_desc, tex_col, texels, mat_tex, prim_uv;             // jp_upload_scene_textured
	DevBuf pick_bins, pick_pmf, pick_env;                            // JP_LIGHTS_POWER_ONE (jp_pick.h)
	DevBuf env_texel, env_bins, env_rows;                            // environment map (jp_env.h)
	DevBuf prim_vn;                                                  // vertex normals (jp_normals.h)
	DevBuf nm_desc, nm_texels, nm_mat, nm_prim_uv;                   // normal maps (jp_normal_map.h)
	DevBuf ts_tex, ts_map;                                           // texture sampling records (jp_tex_sampling.h)
	DevBuf proc_rec, proc_tex;                                       // procedural textures (jp_procedural.h): the records and the per-texture index
	DevBuf mip_tex, mip_lev;                                         // mip maps (jp_mipmap.h): the level tables; the pyramids' texels follow level 0 in `texels`
};
// The arrays behind a Queues view (the fused schedule's region queues have no hit records and no per-block counts)
struct QueueBufs { DevBuf ray_o[2], ray_d[2], beta[2], blk_q[2], hit, lacc, sh_o, sh_d, sh_c, blk_sh; };

// the map jp_set_environment_map copied, waiting for the next upload (W == 0: none)
struct EnvMapHost { int W = 0, H = 0, up = 0, importance = 0; std::vector<float> rgb; };
// the normals jp_set_vertex_normals copied, waiting for the next upload (set false: none)
struct VertexNormalsHost { bool set = false; int n_triangles = 0, n_smooth = 0; std::vector<float> vn; };

// the maps jp_set_normal_maps copied, waiting for the next upload (set false: none); texels already one dword each, neutral: R == G == 128 everywhere
struct NormalMapsHost { bool set = false; int n_materials = 0, n_triangles = 0, n_mapped = 0; std::vector<int> width, height, mat_map; std::vector<long long> first; std::vector<char> neutral;
                        std::vector<unsigned int> texels; std::vector<float> strength, tri_uv; };

// the records jp_set_texture_sampling copied, waiting for the next upload (has_tex / has_map false: none of that kind)
struct TexSamplingHost { bool has_tex = false, has_map = false; int n_textures = 0, n_maps = 0, n_active_textures = 0, n_active_maps = 0; std::vector<JpTexSampler> tex, map; };

// the modes jp_set_texture_mipmaps copied, waiting for the next upload (set false: none)
struct MipmapsHost { bool set = false; int n_textures = 0, n_on = 0; float footprint_scale = 0.f, bounce_spread = 0.f; std::vector<int32_t> mode; };

// the records jp_set_texture_procedurals copied, waiting for the next upload (set false: none)
struct ProceduralsHost { bool set = false; int n_textures = 0, n_on = 0, n_aa = 0; std::vector<JpProcedural> rec; };

struct JpContext
{
	int device = 0;
	JpOptions opt{}, opt_env{};                                    // the options in force; their initial value (defaults + environment, jp_create_context)
	hipStream_t stream = nullptr;
	int n_cus = 256;
	ScenePlan plan; SceneTables tab;                               // scene: what the upload decided, then the device tables behind it
	bool cert_fell_back = false; int cert_eye_leaves = 0;          // certified walk: did the last renders leave it (a result of rendering, cleared at upload)
	int sincosf_mode = 0, libm_mode = 0;
	bool build_on_device = false; float build_ms = 0.f; int bvh_height = 0, bvh_nodes = 0;
	int wide_height = 0, q4_height = 0; size_t tab_bytes[JP_UPLOAD_TABLES] = {};   // levels of the 8-wide / 4-wide trees; bytes in use of every table of the upload (jp_read_scene_table)
	// queues
	Queues q = {}; QueueBufs qb; unsigned int cap = 0; int planes_alloc = 0; unsigned int blk_alloc = 0; int blocks_per_cu = 16;
	DevBuf pix_acc, spill, film;
	DevBuf bsdf_in, bsdf_out, bsdf_fl;                             // jp_bsdf scratch
	DevBuf gamma, rgb8; PinnedBuf h_rgb8;                          // jp_render_rgb8
	PinnedBuf h_film;                                              // pinned staging buffer of jp_render (a pageable copy of the film costs ~2 ms)
	DevBuf cnt;                                                    // one DevCounters
	// timing
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool profiling = false;
	std::vector<hipEvent_t> evpool; size_t evused = 0;
	struct Stamp { int cls; size_t a, b; };
	std::vector<Stamp> stamps;
	JpCounters counters;
	// Extra "lanes": the shard's bands are dealt round-robin to L lanes (this context + L - 1 lane contexts) and rendered
	// concurrently on L streams with L queue sets, so the tail and the launch gap of one lane's kernel are filled by another
	// lane's and bandwidth-bound kernels overlap instruction-bound ones ("Stream lanes").  A lane shares
	// the scene tables (its own `tab` stays empty) and writes its bands into its own film; the films are merged at the end.
	std::vector<JpContext*> lanes; bool is_lane = false; unsigned long long own_samples = 0; bool bpc_from_env = false;
	hipEvent_t ev_added = nullptr; bool added_valid = false; int last_lanes = 1;      // lanes used by the last render (1: this context alone)
	// fused schedule (k_path, jp_path.h): region queues of the resident workgroups, the batch's radiance array, job counters
	Queues fq = {}; QueueBufs fqb; unsigned int fcap = 0; int fplanes = 0;
	DevBuf jobs;
	int last_fused = 0, last_region = 0, last_wgs = 0;
	// textures (jp_upload_scene_textured): the tables belong to the parent context and reach the lanes through `plan.tv` (its side pointer is
	// set per launch); every context owns the side array of its own queue set (k_texel -> k_shade_tex, one word per queue position)
	int n_textures = 0, n_tex_mats = 0; long long texel_bytes = 0; int last_textured = 0;
	DevBuf side;
	// guides and denoising (jp_denoise.h): the filter's per-pixel records (two colour buffers, the normals), the staging area of the host
	// variants, event pairs around the kernels, what the last calls did (jp_get_denoise_info)
	DevBuf dn_cz[2], dn_nr, dn_stage;
	hipEvent_t dn_ev[2] = { nullptr, nullptr }, gd_ev[2] = { nullptr, nullptr }; bool dn_timed = false, gd_timed = false;
	int last_dn = 0, last_dn_demod = 0, last_guide_spp = 0; float last_dn_sigma[3] = { 0.f, 0.f, 0.f };
	// light selection (jp_pick.h): the mode the next upload takes (jp_set_light_sampling), the uploaded scene's table (owned by the parent context,
	// reaches the lanes through `plan.pv`) and what jp_get_light_info reports
	int light_mode = JP_LIGHTS_ALL;
	int n_selectable = 0; double total_weight = 0.0; int last_picked = 0;
	// environment map (jp_env.h): the map the next upload takes (jp_set_environment_map), and what jp_get_env_info reports of the uploaded scene's
	EnvMapHost env_map;
	int env_importance = 0, env_n_selectable = 0; double env_total_weight = 0.0; long long env_table_bytes = 0; int last_mapped = 0;
	// estimator (jp_mis.h): render-time state (jp_set_estimator; a lane takes its parent's before it renders), what the last render ran, and the side records of
	// this context's queue set, one float2 per position of each ray queue, allocated by the first MIS render
	int estimator = JP_ESTIMATOR_NEE, last_mis = 0;
	DevBuf mis_side[2];
	// vertex normals (jp_normals.h): the normals the next upload takes (jp_set_vertex_normals), what jp_get_normal_info reports of the uploaded scene's, and the
	// side records of this context's queue set (k_normal -> k_shade_smooth*, one float4 per queue position)
	VertexNormalsHost vnormals;
	int vn_triangles = 0, vn_smooth = 0, last_smooth = 0; long long vn_table_bytes = 0; double normal_ms = 0.0;   // normal_ms: k_normal's launches of the last render (profiling)
	DevBuf nside;
	// normal maps (jp_normal_map.h): the maps the next upload takes (jp_set_normal_maps) and what jp_get_normal_map_info reports; the side records are nside
	NormalMapsHost nmaps;
	int last_nmapped = 0; double normal_map_ms = 0.0;
	// texture sampling records (jp_tex_sampling.h): the records the next upload takes (jp_set_texture_sampling), the texture count of the upload in progress
	// (jp_upload_scene_textured tells jp_upload_scene; 0 else) and what jp_get_texture_sampling_info reports
	TexSamplingHost tsamp;
	int upload_n_textures = 0, last_sampled = 0; double texel_ms = 0.0;
	// mip maps (jp_mipmap.h): the modes the next upload takes (jp_set_texture_mipmaps), the uploaded scene's level tables as the host keeps them (jp_read_mip_chain), what
	// jp_get_texture_mipmap_info reports, and the ray cones of this context's queue set (k_texel_m, one float2 per path slot, allocated by the first render that needs it)
	MipmapsHost mipmaps;
	std::vector<int2> mip_host_tex; std::vector<JpMipLevel> mip_host_lev; double mip_build_ms = 0.0; int last_mip = 0;
	DevBuf cone;
	// procedural textures (jp_procedural.h): the records the next upload takes (jp_set_texture_procedurals) and what the last render ran
	ProceduralsHost procedurals; int last_proc = 0;
	// thin-lens camera (jp_lens_runtime.h): render-time state like the estimator (jp_set_lens; a lane takes its parent's before it renders) and what the last
	// render ran.  The plan is a kernel argument made per launch from the uploaded camera: the lens owns no device memory.
	JpLens lens = {}; bool lens_on = false; int last_lens = 0;
	// camera projection (jp_projection_runtime.h): render-time state like the lens (jp_set_projection; a lane takes its parent's), what the last render ran and the
	// cone spread it used.  The plan is a kernel argument made per launch from the uploaded camera: a projection owns no device memory.
	JpProjection proj = {}; bool proj_on = false; int last_proj = 0; float last_proj_gamma0 = 0.f;
	// film (jp_film.h): render-time state like the lens -- the film state (jp_set_film; a lane takes its parent's) and the tone map (jp_set_tonemap, resolved:
	// defaults filled in) -- what the last render / transform ran, the histogram's 257 dwords on the device, event pairs around k_film_hist and k_display
	JpFilm film_state = {}; bool film_on = false; int last_hdr = 0;
	JpToneMap tonemap = {}; bool tonemap_on = false; int last_tonemapped = 0; float last_scale = 0.f;
	DevBuf film_hist, film_stage;
	hipEvent_t fh_ev[2] = { nullptr, nullptr }, tm_ev[2] = { nullptr, nullptr }; bool fh_timed = false, tm_timed = false;
	// variance (jp_variance.h): set for the length of a variance render (jp_render_variance*; a lane takes its parent's flag and gets a plane of its own) -- launch_resolve
	// then picks k_resolve_var, which keeps (mean, m2) per pixel in var_mom across batches and writes var_dev; var_plane: the staging plane of the host variants / a lane's
	// plane; the variance-guided filter's second normal + variance buffer (the first is dn_nr), its event pair and what the last calls did (jp_get_variance_info)
	bool var_on = false; float* var_dev = nullptr; int last_var = 0; long long last_mom_bytes = 0;
	DevBuf var_mom, var_plane, dn_nv;
	hipEvent_t dv_ev[2] = { nullptr, nullptr }; bool dv_timed = false;
	int last_dv = 0, last_dv_demod = 0; float last_dv_sigma[3] = { 0.f, 0.f, 0.f };
	// adaptive sampling (jp_adaptive.h): what the last jp_render_adaptive* / jp_adaptive_probe did (jp_get_adaptive_info); its per-pixel state lives in the call
	JpAdaptiveInfo ad_info = {};
};
// jp_pick.h / jp_env.h (included last) define the upload's table steps
static int upload_light_table(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const std::vector<float>& area);
static int upload_environment_map(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, bool pick);
static int upload_vertex_normals(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s);   // jp_normals.h
static int upload_normal_maps(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s);      // jp_normal_map.h
static int check_sampling_counts(const JpContext* c, int n_textures);                               // jp_tex_sampling.h
static int check_sampling_textures(const JpContext* c, const JpTextures* t);
static int upload_map_sampling(JpContext* c, SceneTables& T, ScenePlan& plan);
static int upload_tex_sampling(JpContext* c, SceneTables& T, ScenePlan& plan);
static int check_mipmap_counts(const JpContext* c, int n_textures);                                 // jp_mipmap.h
static int check_mipmap_textures(const JpContext* c, const JpTextures* t, long long pool);
static long long mip_pool_texels(const JpContext* c, const JpTextures* t, long long pool);
static int upload_mipmaps(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const JpTextures* t, const std::vector<int4>& desc, long long pool);
static int ensure_cone(JpContext* c, unsigned int cap, MipView& mv);
static int check_procedural_counts(const JpContext* c, int n_textures);                             // jp_procedural.h
static int check_procedural_textures(const JpContext* c, const JpTextures* t);
static int upload_procedurals(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const JpTextures* t);

// a context buffer that kernels in flight may still use: grown only once the stream is idle (nothing happens when the capacity suffices)
static int reserve_idle(JpContext* c, DevBuf& b, size_t bytes)
{
	if (b.bytes() >= bytes) return JP_OK;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(b.reserve(bytes));
	return JP_OK;
}
static int ensure_film(JpContext* c, size_t n_floats) { return reserve_idle(c, c->film, n_floats * sizeof(float)); }

static void free_scene(JpContext* c)
{
	c->tab = SceneTables();
	c->plan.have_scene = false;
	c->plan.pv = PickView(); c->plan.pick = false; c->n_selectable = 0; c->total_weight = 0.0;
	c->plan.ev = EnvView(); c->plan.env = false; c->plan.env_mean_sum = 0.0; c->env_n_selectable = 0; c->env_total_weight = 0.0; c->env_table_bytes = 0;
	c->plan.tv = TexView(); c->plan.textured = false; c->n_textures = c->n_tex_mats = 0; c->texel_bytes = 0;   // (jp_upload_scene drops the textures of an earlier textured upload)
	c->side.reset();                                               // ... and the side array only textured frames use (callers synchronise first)
	c->plan.nv = NormView(); c->plan.smooth = false; c->vn_triangles = c->vn_smooth = 0; c->vn_table_bytes = 0; c->nside.reset();
	c->plan.mp = NMapView(); c->plan.mapped = false; c->plan.nm_maps = c->plan.nm_mapped = 0; c->plan.nm_texel_bytes = c->plan.nm_table_bytes = 0;
	c->plan.sm = SampView(); c->plan.ts_active_textures = c->plan.ts_active_maps = 0; c->plan.ts_table_bytes = 0;
	c->plan.mv = MipView(); c->plan.mip_on = c->plan.mip_levels = 0; c->plan.mip_bytes = 0; c->mip_host_tex.clear(); c->mip_host_lev.clear(); c->mip_build_ms = 0.0; c->cone.reset();
	// ... and the lanes' cone arrays: sync_lane_scene drops a lane's only when that lane renders again, so a scene rendered in fewer lanes than the one before it
	// would keep -- and jp_get_texture_mipmap_info would report -- cones no render of it needs
	for (JpContext* l : c->lanes) if (l->cone) { hipStreamSynchronize(l->stream); l->cone.reset(); }
	c->plan.proc = ProcView(); c->plan.proc_on = c->plan.proc_aa = 0; c->plan.proc_bytes = 0;
}

// Which build of glibc's sinf / cosf / sincosf does this host run (jp_shading.h, sincosf_libm)?  The reference computes its
// bounce directions with them, so the device reproduces whichever the host's IFUNC resolver picked: 1 = the FMA build,
// 2 = the build without contraction, 0 = neither reproduces the host on the probe set (another libm): the device then
// keeps its own correctly rounded evaluation.
static int probe_host_sincosf()
{
	static int cached = -1;
	if (cached >= 0) return cached;
	bool okF = true, okN = true;
	uint32_t st = 0x12345u;
	for (int i = 0; i < 200000 && (okF || okN); i++)
	{
		st = st * 1664525u + 1013904223u;
		float y;
		if (i < 150000) y = (float)(st >> 8) * (1.0f / 16777216.0f) * 6.2831855f;      // the call sites' range [0, 2 pi)
		else if (i < 180000) y = (float)(st >> 8) * (1.0f / 16777216.0f) * 0.01f;       // small arguments, incl. the < 2^-12 branch
		else y = ((float)(st >> 8) * (1.0f / 16777216.0f) - 0.5f) * 200.f;               // both signs, up to |y| = 100
		float hs, hc; ::sincosf(y, &hs, &hc);
		const float h1 = ::sinf(y), h2 = ::cosf(y);
		float as, ac, bs, bc;
		jp::sincosf_libm<true>(y, &as, &ac); jp::sincosf_libm<false>(y, &bs, &bc);
		uint32_t uhs, uhc, u1, u2, uas, uac, ubs, ubc;
		std::memcpy(&uhs, &hs, 4); std::memcpy(&uhc, &hc, 4); std::memcpy(&u1, &h1, 4); std::memcpy(&u2, &h2, 4);
		std::memcpy(&uas, &as, 4); std::memcpy(&uac, &ac, 4); std::memcpy(&ubs, &bs, 4); std::memcpy(&ubc, &bc, 4);
		if (uhs != u1 || uhc != u2) { okF = okN = false; }                             // sinf / cosf / sincosf must agree with each other
		if (uas != uhs || uac != uhc) okF = false;
		if (ubs != uhs || ubc != uhc) okN = false;
	}
	cached = okF ? 1 : (okN ? 2 : 0);
	return cached;
}

// Do jp_libm.h's logf / expf / powf / acosf / atanf / tanf reproduce the host's libm (jp_xbsdf.h: g_libm_mode)?  Bit 0: all six do on
// every probe argument; bit 1: with the FMA build of the first three (glibc's IFUNC picks it on CPUs with FMA + AVX2; the two builds
// differ on about one argument in 10^8, so the CPU feature decides and the probe confirms).  0: another libm -- the device keeps its
// own library for these functions (k_bsdf then matches the reference within the tolerance of tests/test_gpu_parity.py, not bit for bit).
static int probe_host_libm()
{
	static int cached = -1;
	if (cached >= 0) return cached;
	bool fma_cpu = false;
#if defined(__x86_64__)
	fma_cpu = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#endif
	auto same = [](float a, float b) { uint32_t x, y; std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4); return x == y || (a != a && b != b); };
	auto run = [&](bool fmab) {
		uint32_t st = 0x2545f491u;
		auto rnd = [&]() { st = st * 1664525u + 1013904223u; return st; };
		auto u01 = [&]() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); };
		for (int i = 0; i < 200000; i++)
		{
			float x, y;
			switch (i & 3)
			{
			case 0: { const uint32_t a = rnd(), b = rnd(); std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4); break; }   // raw bit patterns: every exponent, specials
			case 1: x = u01(); y = u01() * 8.f; break;                                                                  // the call sites' ranges
			case 2: x = (u01() - 0.5f) * 250.f; y = (u01() - 0.5f) * 64.f; break;
			default: x = u01() * 1e-3f; y = 1.f / (u01() * 100.f + 1.f); break;
			}
			const float e = fmab ? jp::lm::expf_libm<true>(x) : jp::lm::expf_libm<false>(x), l = fmab ? jp::lm::logf_libm<true>(x) : jp::lm::logf_libm<false>(x);
			const float pw = fmab ? jp::lm::powf_libm<true>(x, y) : jp::lm::powf_libm<false>(x, y);
			if (!same(e, ::expf(x)) || !same(l, ::logf(x)) || !same(pw, ::powf(x, y))) return false;
			const float a = (i & 3) == 0 ? x : x * 2.f - 1.f;
			if (!same(jp::lm::acosf_libm(a), ::acosf(a)) || !same(jp::lm::atanf_libm(x), ::atanf(x))) return false;
			bool ok; const float t = jp::lm::tanf_libm(x * 8.f, &ok);
			if (ok && !same(t, ::tanf(x * 8.f))) return false;
		}
		return true;
	};
	int mode = 0;
	if (run(fma_cpu)) mode = 1 | (fma_cpu ? 2 : 0);
	else if (run(!fma_cpu)) mode = 1 | (fma_cpu ? 0 : 2);
	cached = mode;
	return cached;
}

// gamma_encoding of film.h:24 exactly as the host computes it (std::pow on floats = powf, product in double, truncation)
static inline unsigned char host_gamma_encoding(float x)
{
	const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
	return (unsigned char)(std::pow(c, (float)(1 / 2.2)) * 255.0);
}
// thr[k-1] = smallest fp32 x in [0, 1] with host_gamma_encoding(x) >= k, k = 1..255: the floats of [0, 1] are ordered like
// their bit patterns and the encoding is non-decreasing, so each threshold is a binary search over 0 .. 0x3f800000
static const float* host_gamma_thresholds()
{
	static float thr[255]; static std::once_flag once;
	std::call_once(once, []() {
		for (int k = 1; k <= 255; k++)
		{
			uint32_t lo = 0, hi = 0x3f800000u;                       // enc(lo) < k (enc(0) = 0) ... enc(hi) >= k (enc(1) = 255)
			while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; float f; std::memcpy(&f, &mid, 4); if (host_gamma_encoding(f) >= k) hi = mid; else lo = mid; }
			std::memcpy(&thr[k - 1], &hi, 4);
		}
	});
	return thr;
}
// The binary search above assumes that the host's powf-based encoding never steps DOWN on [0, 1] (powf is accurate to under an ulp, not
// guaranteed monotone).  This sweeps EVERY float bit pattern of [0, 1] -- 1,065,353,217 values, n_threads host threads -- and counts
// the values whose byte differs from (number of thresholds <= x): 0 means the device tone map is byte-identical to gamma_encoding for
// every input (tests/test_host_and_abi.py).
static unsigned long long host_gamma_sweep(int n_threads)
{
	const float* thr = host_gamma_thresholds();
	n_threads = std::max(1, std::min(64, n_threads));
	std::vector<unsigned long long> bad((size_t)n_threads, 0ull);
	std::vector<std::thread> pool;
	const uint64_t total = 0x3f800000ull + 1;
	for (int t = 0; t < n_threads; t++)
		pool.emplace_back([&, t]() {
			const uint64_t a = total * t / n_threads, b = total * (t + 1) / n_threads;
			int k = 0;                                                    // thresholds <= x: x ascends, so k only grows
			{ const uint32_t u = (uint32_t)a; float f; std::memcpy(&f, &u, 4); while (k < 255 && thr[k] <= f) k++; }
			unsigned long long nb = 0;
			for (uint64_t i = a; i < b; i++)
			{
				const uint32_t u = (uint32_t)i; float f; std::memcpy(&f, &u, 4);
				while (k < 255 && thr[k] <= f) k++;
				if (host_gamma_encoding(f) != (unsigned char)k) nb++;
			}
			bad[(size_t)t] = nb;
		});
	for (auto& th : pool) th.join();
	unsigned long long s2 = 0; for (unsigned long long v : bad) s2 += v;
	return s2;
}

// a caller's JpOptions by value: a longer struct of a later ABI is truncated, a shorter one zero-extended; every field range-checked
static int read_options(const char* who, const JpOptions* o, JpOptions& n)
{
	if (o->struct_bytes < (int32_t)sizeof(int32_t) || o->struct_bytes > 4096) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": struct_bytes is not a struct size");
	std::memset(&n, 0, sizeof(n));
	std::memcpy(&n, o, std::min<size_t>(sizeof(n), (size_t)o->struct_bytes));
	n.struct_bytes = (int32_t)sizeof(JpOptions);
	if (n.lanes < 0 || n.lanes > 4 || n.lane_rows < 0 || n.lane_rows > 64 || n.blocks_per_cu < 0 || n.blocks_per_cu > 256 || n.max_slots < 0 || n.traversal < 0 || n.traversal > 4
	    || n.stack_lds_words < 0 || n.bvh_max_leaf < 0 || n.bvh_max_leaf > 16 || n.trace_walk < 0 || n.trace_walk > 3 || n.device_tree < 0 || n.device_tree > 2
	    || (n.persist > 0 && n.persist != 8 && n.persist != 16 && n.persist != 32))
		return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": field out of range (see JpOptions in jetpbrt_amd.h)");
	return JP_OK;
}

extern "C" {

const char* jp_last_error(void) { return g_err.c_str(); }
int jp_gamma_thresholds(float* out255) { if (!out255) return fail(JP_ERR_INVALID_ARGUMENT, "jp_gamma_thresholds: null argument"); std::memcpy(out255, host_gamma_thresholds(), 255 * sizeof(float)); return JP_OK; }
int jp_abi_version(void) { return JP_ABI_VERSION; }
long long jp_gamma_sweep(int n_threads) { return (long long)host_gamma_sweep(n_threads); }
int jp_probe_libm_sincosf(void) { return probe_host_sincosf(); }
int jp_probe_libm_xbsdf(void) { return probe_host_libm(); }

int jp_create_context(int device_id, JpContext** out)
{
	if (!out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_create_context: out is null");
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(JP_ERR_NO_DEVICE, "jp_create_context: no HIP device visible (this library has no CPU fallback)");
	if (device_id < 0 || device_id >= n) return fail(JP_ERR_NO_DEVICE, "jp_create_context: device id out of range");
	HIP_TRY(hipSetDevice(device_id));
	JpContext* c = new JpContext;
	c->device = device_id;
	std::memset(&c->counters, 0, sizeof(c->counters));
	std::memset(&c->q, 0, sizeof(c->q));
	std::memset(&c->opt_env, 0, sizeof(JpOptions)); c->opt_env.struct_bytes = (int32_t)sizeof(JpOptions);
	options_from_environment(c->opt_env);
	c->opt = c->opt_env;
	if (c->opt.blocks_per_cu >= 1 && c->opt.blocks_per_cu <= 256) { c->blocks_per_cu = c->opt.blocks_per_cu; c->bpc_from_env = true; }
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cus = prop.multiProcessorCount;
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess
	    || c->cnt.reserve(sizeof(DevCounters)) != hipSuccess)
	{ jp_destroy_context(c); return fail(JP_ERR_DEVICE, "jp_create_context: stream/event/counter allocation failed"); }
	c->sincosf_mode = c->opt.libm_sincosf == 0 ? probe_host_sincosf() : (c->opt.libm_sincosf < 0 ? 0 : std::min(2, c->opt.libm_sincosf));
	{ hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(jp::g_sincosf_mode), &c->sincosf_mode, sizeof(int)); if (e != hipSuccess) { jp_destroy_context(c); return fail(JP_ERR_DEVICE, std::string("jp_create_context: hipMemcpyToSymbol: ") + hipGetErrorString(e)); } }
	c->libm_mode = c->opt.libm_xbsdf == 0 ? probe_host_libm() : (c->opt.libm_xbsdf < 0 ? 0 : (c->opt.libm_xbsdf & 3));
	{ hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(jp::xb::g_libm_mode), &c->libm_mode, sizeof(int)); if (e != hipSuccess) { jp_destroy_context(c); return fail(JP_ERR_DEVICE, std::string("jp_create_context: hipMemcpyToSymbol: ") + hipGetErrorString(e)); } }
	*out = c;
	return JP_OK;
}

// ABI 7: options by value.  Schedule fields take effect with the next jp_render*, traversal fields with the next jp_upload_scene; the libm fields
// re-select the device's transcription at once.  NULL restores the initial value (defaults + environment).
int jp_set_options(JpContext* c, const JpOptions* o)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_options: null context");
	JpOptions n = c->opt_env;
	if (o) if (const int st = read_options("jp_set_options", o, n); st != JP_OK) return st;
	const bool libm_changed = n.libm_sincosf != c->opt.libm_sincosf || n.libm_xbsdf != c->opt.libm_xbsdf;
	c->opt = n;
	c->blocks_per_cu = (n.blocks_per_cu >= 1) ? n.blocks_per_cu : 16; c->bpc_from_env = n.blocks_per_cu >= 1;
	for (JpContext* l : c->lanes) { l->blocks_per_cu = c->blocks_per_cu; l->opt = c->opt; }
	if (libm_changed)
	{
		HIP_TRY(hipSetDevice(c->device));
		c->sincosf_mode = n.libm_sincosf == 0 ? probe_host_sincosf() : (n.libm_sincosf < 0 ? 0 : std::min(2, n.libm_sincosf));
		c->libm_mode = n.libm_xbsdf == 0 ? probe_host_libm() : (n.libm_xbsdf < 0 ? 0 : (n.libm_xbsdf & 3));
		HIP_TRY(hipStreamSynchronize(c->stream));
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(jp::g_sincosf_mode), &c->sincosf_mode, sizeof(int)));
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(jp::xb::g_libm_mode), &c->libm_mode, sizeof(int)));
	}
	return JP_OK;
}
int jp_get_options(JpContext* c, JpOptions* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_options: null argument");
	*out = c->opt; out->struct_bytes = (int32_t)sizeof(JpOptions);
	return JP_OK;
}

int jp_destroy_context(JpContext* c)
{
	if (!c) return JP_OK;
	hipSetDevice(c->device);
	if (c->stream) hipStreamSynchronize(c->stream);
	for (JpContext* l : c->lanes) jp_destroy_context(l);
	c->lanes.clear();
	for (hipEvent_t e : { c->ev_added, c->dn_ev[0], c->dn_ev[1], c->gd_ev[0], c->gd_ev[1], c->fh_ev[0], c->fh_ev[1], c->tm_ev[0], c->tm_ev[1], c->dv_ev[0], c->dv_ev[1], c->ev0, c->ev1 }) if (e) hipEventDestroy(e);
	for (hipEvent_t e : c->evpool) hipEventDestroy(e);
	if (c->stream) hipStreamDestroy(c->stream);
	delete c;                                                      // every DevBuf / PinnedBuf member frees its memory
	return JP_OK;
}
long long jp_device_bytes_in_use(void) { return g_device_bytes.load(); }

} // extern "C"

