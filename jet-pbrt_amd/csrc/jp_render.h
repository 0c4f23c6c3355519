// jet-pbrt_amd/csrc/jp_render.h -- host runtime, part 3 of 3: jp_render* -- the shard helper, the kernel selectors (k_shade's launcher: jp_shade_launch.h), queue budget, the per-bounce launch sequence, stream lanes, the fused schedule,
// and the rest of the C ABI (counters, build info, jp_trace, jp_bsdf, tone map).  Every buffer is a DevBuf of the context (grown through reserve_idle, jp_runtime.h, when
// kernels in flight may use it) or a local DevBuf of the call; ensure_queues regrows a queue set as a whole.  Included by jp_kernels.hip after jp_upload.h.
#pragma once
// ---- render ---------------------------------------------------------------------------------------------------------------
namespace
{
enum { CLS_EXTEND = 0, CLS_SHADE = 1, CLS_SHADOW = 2, CLS_OTHER = 3, CLS_PATH = 4, CLS_NORMAL = 5, CLS_NMAP = 6, CLS_TEXEL = 7, CLS_ADAPT_SELECT = 8, CLS_ADAPT_RESOLVE = 9 };   // (CLS_NORMAL: k_normal, stamped inside its CLS_SHADE pair -- a share of shade_ms, JpNormalInfo)

// the lens in force as the kernels take it (zeros while none is set: the kernels then do not read it); the camera is the uploaded scene's
int lens_plan_of(const JpContext* c, JpLensPlan& lp)
{
	std::memset(&lp, 0, sizeof(lp));
	if (!c->lens_on) return JP_OK;
	if (jp_lens_make_plan(&c->plan.sv.cam, &c->lens, &lp) != 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: the uploaded camera's right / up vectors have no finite positive length");
	return JP_OK;
}

// the projection in force as the kernels take it (zeros, kind 0, while none is set: the pinhole), with the checks that need the uploaded camera
int proj_plan_status(const JpCamera* cam, const JpProjection* pr, JpProjectionPlan& pp, const char* who)
{
	switch (jp_projection_make_plan(cam, pr, &pp))
	{
	case 0: return JP_OK;
	case -1: return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": the camera's right / up / front vectors need a finite positive length and the resolution must be positive");
	default: return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": an equirectangular or fisheye projection needs perpendicular camera axes (a pairwise |dot| of right, up, front, normalised, exceeds 1e-3)");
	}
}
int proj_plan_of(const JpContext* c, JpProjectionPlan& pp)
{
	std::memset(&pp, 0, sizeof(pp));
	if (!c->proj_on) return JP_OK;
	if (c->lens_on) return fail(JP_ERR_UNSUPPORTED, "jp_set_projection: a lens (jp_set_lens, radius > 0) together with a projection other than perspective is not supported");
	return proj_plan_status(&c->plan.sv.cam, &c->proj, pp, "jp_set_projection");
}

void free_queues(JpContext* c) { c->qb = QueueBufs(); c->cap = 0; c->planes_alloc = 0; c->blk_alloc = 0; }

int ensure_queues(JpContext* c, unsigned int cap, int planes, unsigned int nblocks)
{
	if (c->cap >= cap && c->planes_alloc >= planes && c->blk_alloc >= nblocks) return JP_OK;
	cap = std::max(cap, c->cap); planes = std::max(planes, c->planes_alloc); nblocks = std::max(nblocks, c->blk_alloc);
	free_queues(c);                                                  // all or nothing: the whole set goes before the larger one is allocated
	auto alloc = [](DevBuf& b, auto*& p, size_t bytes) { return reserve(b, p, bytes) == hipSuccess; };
	Queues& q = c->q; QueueBufs& qb = c->qb; bool ok = true;
	for (int b = 0; b < 2 && ok; b++) ok = alloc(qb.ray_o[b], q.ray_o[b], (size_t)cap * 16) && alloc(qb.ray_d[b], q.ray_d[b], (size_t)cap * 16) && alloc(qb.beta[b], q.beta[b], (size_t)cap * 16)
	                                       && alloc(qb.blk_q[b], q.blk_q[b], (size_t)nblocks * 4);
	ok = ok && alloc(qb.hit, q.hit, (size_t)cap * 8) && alloc(qb.lacc, q.lacc, (size_t)cap * 16) && alloc(qb.sh_o, q.sh_o, (size_t)cap * 16)
	     && alloc(qb.sh_d, q.sh_d, (size_t)cap * 16 * planes) && alloc(qb.sh_c, q.sh_c, (size_t)cap * 16 * planes) && alloc(qb.blk_sh, q.blk_sh, (size_t)nblocks * 4);
	if (!ok) { free_queues(c); return fail(JP_ERR_DEVICE, "jp_render: out of device memory for the path queues"); }
	c->cap = cap; c->planes_alloc = planes; c->blk_alloc = nblocks;
	return JP_OK;
}

int ensure_gamma(JpContext* c)
{
	if (!c->gamma) HIP_TRY(upload(c->gamma, host_gamma_thresholds(), 255 * sizeof(float)));
	return JP_OK;
}
// the 8-bit film of n bytes and the gamma table, then k_tonemap8: n floats at src -> c->rgb8, on the context's stream
int ensure_rgb8(JpContext* c, size_t n)
{
	if (const int e = reserve_idle(c, c->rgb8, n); e != JP_OK) return e;
	return ensure_gamma(c);
}
void tonemap8(JpContext* c, const float* src, size_t n)
{
	hipLaunchKernelGGL(k_tonemap8, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream, src, c->rgb8.get<unsigned char>(), c->gamma.get<const float>(), n);
}

// k_resolve of one batch, for both schedules: the film instance while a film state is in force (jp_set_film), else the kernel that always ran
// a variance render's per-frame state: the (zero) variance plane and the moments of this context's npix pixels (nothing while none runs)
int variance_begin(JpContext* c, const JpRenderParams* rp, long long npix)
{
	if (!c->var_on) return JP_OK;
	HIP_TRY(hipMemsetAsync(c->var_dev, 0, sizeof(float) * (size_t)rp->width * rp->height, c->stream));
	return reserve_idle(c, c->var_mom, (size_t)std::max<long long>(npix, 1) * sizeof(float2));
}

void launch_resolve(JpContext* c, const Queues& q, const RenderConst& rc, long long npix, float4* pix_acc, float* film_dev, int first, int last)
{
	const dim3 grid((unsigned int)std::min<long long>(c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK));
	if (c->var_on)
	{   // a variance render (jp_variance.h): the twin that also keeps the moments; without a film state it writes k_resolve's film (hdr 0, no clamp)
		hipLaunchKernelGGL(k_resolve_var, grid, dim3(JP_BLOCK), 0, c->stream, q, rc, pix_acc, film_dev, c->var_mom.get<float2>(), c->var_dev, first, last,
		                   c->film_on ? c->film_state.hdr : 0, c->film_on ? c->film_state.sample_clamp : 0.f);
		if (c->film_on) c->last_hdr = 1;
	}
	else if (c->film_on) { hipLaunchKernelGGL(k_resolve_film, grid, dim3(JP_BLOCK), 0, c->stream, q, rc, pix_acc, film_dev, first, last, c->film_state.hdr, c->film_state.sample_clamp); c->last_hdr = 1; }
	else hipLaunchKernelGGL(k_resolve, grid, dim3(JP_BLOCK), 0, c->stream, q, rc, pix_acc, film_dev, first, last);
}

struct Stamper
{
	JpContext* c; int cls; size_t a;
	Stamper(JpContext* c, int cls) : c(c), cls(cls), a(0)
	{
		if (!c->profiling) return;
		if (c->evused + 2 > c->evpool.size()) { size_t old = c->evpool.size(); c->evpool.resize(old + 64); for (size_t i = old; i < c->evpool.size(); i++) hipEventCreate(&c->evpool[i]); }
		a = c->evused; c->evused += 2;
		hipEventRecord(c->evpool[a], c->stream);
	}
	~Stamper() { if (!c->profiling) return; hipEventRecord(c->evpool[a + 1], c->stream); JpContext::Stamp s = { cls, a, a + 1 }; c->stamps.push_back(s); }
};

// k_texel, or its twin k_texel_s where a colour texture of the scene has an active sampling record (jp_tex_sampling.h); with profiling, timed inside the CLS_SHADE pair
// ... or k_texel_m where one has a pyramid (jp_mipmap.h; mv.cone: this context's cone array)
static void launch_texel(JpContext* c, const ScenePlan& p, int grid, int cur, const TexView& tv, const MipView& mv)
{
	Stamper t(c, CLS_TEXEL);
	if (p.proc_on > 0) hipLaunchKernelGGL(k_texel_p, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, tv, p.sm, mv, p.proc);   // a procedural record (jp_procedural.h): first; mv.cone and mv.tex may each be null
	else if (mv.tex) hipLaunchKernelGGL(k_texel_m, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, tv, p.sm, mv);
	else if (p.sm.tex) hipLaunchKernelGGL(k_texel_s, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, tv, p.sm);
	else hipLaunchKernelGGL(k_texel, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, tv);
}
// k_normal, or a mapped scene's k_normal_map / k_normal_map_s, timed likewise (defined in jp_shade_launch.h: the kernels come after this file)
static void launch_normal(JpContext* c, const ScenePlan& p, int grid, int cur, const NormView& nv);

// ---- the shard: JpRenderParams checked, its bands' rows counted, a lane's share of them ----------------------------------
struct Shard { int band, count, index, local_rows, lane_rows; };     // local_rows: rows of the shard's bands; lane_rows: the ones this lane renders
int shard_of(const JpRenderParams* rp, Shard& s, int lane_index = 0, int lane_count = 1, int lane_group = 4)
{
	if (rp->width <= 0 || rp->height <= 0 || rp->spp <= 0 || rp->max_depth < 0 || rp->max_depth > 200) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: bad width/height/spp/max_depth");
	if (rp->integrator < JP_INTEGRATOR_PATH || rp->integrator > JP_INTEGRATOR_DEBUG_NORMAL) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: unknown integrator");
	if (rp->integrator == JP_INTEGRATOR_WHITTED && rp->max_depth > JP_WHITTED_MAX_DEPTH) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator supports max_depth <= 16");
	if (rp->sampler_mode != JP_SAMPLER_COUNTER && rp->sampler_mode != JP_SAMPLER_DEBUG) return fail(JP_ERR_UNSUPPORTED, "jp_render: the device path implements the counter sampler only (the sequential mt19937_64 stream is not reproducible in parallel)");
	s.band = rp->band_rows > 0 ? rp->band_rows : 20;
	s.count = rp->shard_count > 1 ? rp->shard_count : 1;
	s.index = s.count > 1 ? rp->shard_index : 0;
	if (s.index < 0 || s.index >= s.count) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: shard_index out of range");
	const int nbands = (rp->height + s.band - 1) / s.band;
	s.local_rows = 0;
	for (int b = s.index; b < nbands; b += s.count) s.local_rows += std::min(s.band, rp->height - b * s.band);
	s.lane_rows = 0;      // this lane's share of the shard's rows: groups of lane_group rows dealt round-robin (only the shard's last group can be short; one lane: all of them)
	for (int g0 = lane_index * lane_group; g0 < s.local_rows; g0 += lane_count * lane_group) s.lane_rows += std::min(lane_group, s.local_rows - g0);
	return JP_OK;
}

// ---- kernel selectors: one function per kernel family (path_kernel below is k_path's), the only place of the host code that names the family's instantiations.
// Each returns the kernel with the dynamic LDS and the stack words it is launched with: a pure function of the plan (shadow: and the region size), called once per render.
// (k_shade's families are defined after this file: shade_choice picks here, shade_launch names the instances in jp_shade_launch.h.)
inline bool refill_walks(const ScenePlan& p) { return p.persist && (p.trav_mode == 0 || p.trav_mode == 3 || p.trav_mode == 5); }   // the lane refill kernels exist for these walks
inline int refill_row(const ScenePlan& p) { return p.persist >= 32 ? 2 : (p.persist >= 16 ? 1 : 0); }   // refill threshold 8 / 16 / 32: the row of a walk's table
// stack words a thread's walk may need: closest-hit rays, shadow rays, and the deepest walk of all (the spill area's size)
inline int extend_depth(const ScenePlan& p) { return (p.trav_mode == 5 ? p.cert : p.use_q4) ? p.stack_depth_q4 : p.stack_depth; }
inline int shadow_depth(const ScenePlan& p) { return (p.trav_mode == 5 ? p.cert : p.q4_shadow) ? p.stack_depth_q4 : (p.trav_mode == 3 ? (int)(p.lds_bytes_shadow / (JP_BLOCK * sizeof(int))) : p.stack_depth); }
inline int deepest_walk(const ScenePlan& p) { return std::max(std::max(p.stack_depth, p.stack_depth_q4), p.trav_mode == 3 ? (int)(p.lds_bytes_shadow / (JP_BLOCK * sizeof(int))) : 0); }
// spill area of the walkers' stacks: the words G workgroups' threads may need beyond the ones kept in LDS (+1: Walker<4> keeps one LDS word as a dump slot)
inline size_t spill_need(const ScenePlan& p, int deep, unsigned int G) { return deep >= p.stack_lds_words ? (size_t)(deep - p.stack_lds_words + 1) * G * JP_BLOCK : 1; }

// Feature sets (jp_device.h): the tiny-scene kernels exist a second time without the code a scene of flat shapes (FeatFlat: k_extend<2>,
// k_shadow<2>) lit by area lights on them and made of matte / metal only (FeatLean: k_shade<true, true, true, kSort>) cannot reach.  The plan says what the
// scene holds; `generic` (JpOptions::reserved[0] == 1: tests, A/B runs) keeps the instances with everything in them, which every other scene gets anyway.
inline bool flat_shapes_only(int shape_mask) { return (shape_mask & ~((1 << JP_SHAPE_TRIANGLE) | (1 << JP_SHAPE_RECTANGLE))) == 0; }
inline bool lean_traversal(const ScenePlan& p, bool generic) { return !generic && p.trav_mode == 2 && flat_shapes_only(p.shape_mask); }
inline bool lean_shading(const ScenePlan& p, bool generic)
{
	const int delta_classes = (2 << JP_MAT_MIRROR) | (2 << JP_MAT_GLASS) | (2 << JP_MAT_PLASTIC);      // class_mask: bit 0 none, bit 1 + JP_MAT_*
	return !generic && p.shade_prims_in_lds && p.stage_nee && flat_shapes_only(p.shape_mask) && (p.light_mask & ~(1 << JP_LIGHT_AREA)) == 0
	    && flat_shapes_only(p.light_shape_mask) && (p.class_mask & delta_classes) == 0;
}

typedef void (*ExtendKernel)(SceneView, Queues, int, int, DevCounters*);
inline size_t pool_lds_bytes() { return (size_t)(JP_BLOCK / 64) * JP_POOL_WAVE_BYTES; }   // k_extend_pool / k_trace_pool: the pooled pass's LDS of a workgroup (jp_device.h)
typedef void (*ExtendRefillKernel)(SceneView, Queues, int, int, int*, DevCounters*);
struct ExtendLaunch { ExtendRefillKernel refill; ExtendKernel plain; size_t lds; int words; };   // one of the two kernels; words: of the stack, kept in LDS (refill) / in all (plain)
template <int M> ExtendRefillKernel extend_refill(const ScenePlan& p)
{
	static const ExtendRefillKernel k[3][2] = { { k_extend_persist<M, 8, false>, k_extend_persist<M, 8, true> }, { k_extend_persist<M, 16, false>, k_extend_persist<M, 16, true> }, { k_extend_persist<M, 32, false>, k_extend_persist<M, 32, true> } };
	return k[refill_row(p)][p.vote];
}
ExtendLaunch extend_kernel(const ScenePlan& p, bool generic)
{
#ifndef JP_NO_EXTEND_POOL
	// the wave's primitive tests from one pooled list (k_extend_pool): the 32-bit-mask scenes; its per-wave rays, slots and ring lie behind the primitive table
	if (lean_traversal(p, generic) && p.sv.n_prims <= 32) return { nullptr, k_extend_pool, p.lds_bytes + pool_lds_bytes(), p.stack_depth };
#endif
	if (lean_traversal(p, generic)) return { nullptr, k_extend<2, FeatFlat>, p.lds_bytes, p.stack_depth };
	if (!refill_walks(p)) return { nullptr, p.trav_mode == 5 ? k_extend<5> : (p.trav_mode == 2 ? k_extend<2> : (p.trav_mode == 1 ? k_extend<1> : k_extend<0>)), p.lds_bytes, p.stack_depth };
	const int words = std::min(extend_depth(p), p.stack_lds_words);
	const ExtendRefillKernel k = p.trav_mode == 5 ? (p.cert ? extend_refill<6>(p) : extend_refill<5>(p)) : (p.use_q4 ? extend_refill<4>(p) : extend_refill<0>(p));
	return { k, nullptr, (size_t)words * JP_BLOCK * sizeof(int), words };
}

typedef void (*ShadowKernel)(SceneView, Queues, RenderConst, int, DevCounters*);
typedef void (*ShadowRefillKernel)(SceneView, Queues, RenderConst, int, int*, DevCounters*);
struct ShadowLaunch { ShadowRefillKernel refill; ShadowKernel plain; size_t lds; int words; bool cert_fell_back; };   // cert_fell_back: a certified scene whose shadow rays do not get the certified walk
template <int M> ShadowRefillKernel shadow_refill(const ScenePlan& p)
{
	static const ShadowRefillKernel k[3][2] = { { k_shadow_persist<M, 8, false>, k_shadow_persist<M, 8, true> }, { k_shadow_persist<M, 16, false>, k_shadow_persist<M, 16, true> }, { k_shadow_persist<M, 32, false>, k_shadow_persist<M, 32, true> } };
	return k[refill_row(p)][p.vote];
}
ShadowLaunch shadow_kernel(const ScenePlan& p, unsigned int R, bool generic)   // R: slots per region (Queues::R), whose shadow bitmap shares the refill kernel's LDS with the stacks
{
	const int words = std::min(shadow_depth(p), p.stack_lds_words);
	const size_t plds = (size_t)words * JP_BLOCK * sizeof(int) + (((size_t)R * p.n_planes + 31) / 32) * 4 * (p.cert ? 2 : 1);   // (certified walk: a second bitmap, the rays without a certificate)
#ifndef JP_NO_SHADOW_PAIR
	// two rays of an entry in one pass (k_shadow_pair): the 32-bit-mask scenes whose entries can hold two rays
	if (lean_traversal(p, generic) && p.sv.n_prims <= 32 && p.n_planes >= 2) return { nullptr, k_shadow_pair, p.lds_bytes, p.stack_depth, p.cert };
#endif
	if (lean_traversal(p, generic)) return { nullptr, k_shadow<2, FeatFlat>, p.lds_bytes, p.stack_depth, p.cert };
	if (!refill_walks(p) || plds > 64 * 1024)                         // one ray per lane: these kernels walk a certified scene's caller's tree verbatim
		return { nullptr, p.trav_mode == 3 ? k_shadow<3> : (p.trav_mode == 5 ? k_shadow<5> : (p.trav_mode == 2 ? k_shadow<2> : (p.trav_mode == 1 ? k_shadow<1> : k_shadow<0>))), p.trav_mode == 3 ? p.lds_bytes_shadow : p.lds_bytes, p.stack_depth, p.cert };
	const ShadowRefillKernel k = p.trav_mode == 5 ? (p.cert ? shadow_refill<6>(p) : shadow_refill<5>(p)) : (p.q4_shadow ? shadow_refill<4>(p) : (p.trav_mode == 3 ? shadow_refill<3>(p) : shadow_refill<0>(p)));
	return { k, nullptr, plds, words, false };
}

// k_shade and its families (shade_body<...>: jp_kernels.hip, jp_pick.h, jp_env.h, jp_mis.h, jp_normals.h).  shade_choice says which instance a render runs: a pure function of
// the plan and of what the render switches on.  shade_launch (jp_shade_launch.h, included after the last family) binds that instance to the render's views: the only place
// of the host code that names the instantiations.  Every instance takes plan.shade_lds_bytes.
enum { SHADE_PLAIN = 0, SHADE_LEAN, SHADE_LEAN_ONE, SHADE_PICK, SHADE_ENV, SHADE_MIS, SHADE_MIS_ENV };
enum { ROW_TTT = 0, ROW_TTF, ROW_TFT, ROW_TFF, ROW_FFF };            // <kTab, kPrims, kStage>
struct ShadeChoice { int family; bool tex, smooth; int row; bool sort; };   // (smooth: the family's twin with kSmooth, which exists for sort alone -- the upload plans a smooth scene onto ROW_FFF)
ShadeChoice shade_choice(const ScenePlan& p, bool tex, bool mis, bool smooth, bool generic)
{
	ShadeChoice c;
	c.family = mis ? (p.env ? SHADE_MIS_ENV : SHADE_MIS) : (p.env ? SHADE_ENV : (p.pick ? SHADE_PICK : SHADE_PLAIN));
	c.tex = tex; c.smooth = smooth; c.sort = p.shade_sort;
	c.row = p.shade_prims_in_lds ? (p.stage_nee ? ROW_TTT : ROW_TTF) : (p.tables_in_lds ? (p.stage_nee ? ROW_TFT : ROW_TFF) : ROW_FFF);
	if (c.family == SHADE_PLAIN && !tex && !smooth && lean_shading(p, generic))
	{   // FeatLean (its row is ROW_TTT); the textured twin stays generic (a textured scene is outside the lean sets' measurements)
		c.family = SHADE_LEAN;
#ifndef JP_NO_ONE_SWEEP
		if (p.shade_sort && !p.has_null_material) c.family = SHADE_LEAN_ONE;   // one-sweep partition: a miss does nothing in this instance only while no primitive is without a material
#endif
	}
	return c;
}
// the views of one render, in the order the kernels append them; each kernel takes the ones its signature names (TexView::side, MisView and NormView::side are the queue set's)
typedef std::tuple<TexView, PickView, EnvView, MisView, NormView> ShadeViews;
typedef std::function<void(hipStream_t, int, size_t, const SceneView&, const Queues&, const RenderConst&, int, DevCounters*)> ShadeLaunch;   // (stream, grid, lds, sv, q, rc, cur, cnt)
ShadeLaunch shade_launch(const ShadeChoice& c, const ShadeViews& views);
}
// the bytes of jp_render_rgb8 / jp_render_denoised, after ensure_rgb8: k_tonemap8, or the display transform while a tone map is in force (jp_film.h, part 2)
static int film_to_rgb8(JpContext* c, const float* src, int width, int height);
static int ensure_mis_side(JpContext* c, unsigned int cap, MisView& mv);
static int ensure_normal_side(JpContext* c, unsigned int cap, NormView& nv);
namespace
{

// the other two integrators' megakernel: one ray per lane, launched like the plain k_extend (plan.lds_bytes, plan.stack_depth)
typedef void (*OtherKernel)(SceneView, Queues, RenderConst, int, int, DevCounters*, int, JpLensPlan, JpProjectionPlan);
OtherKernel other_kernel(const ScenePlan& p) { return p.trav_mode == 5 ? k_other<5> : (p.trav_mode == 2 ? k_other<2> : (p.trav_mode == 1 ? k_other<1> : k_other<0>)); }

// jp_trace / jp_surface.  JpOptions::trace_walk (tests; jp_surface passes 0): 1 the binary tree, 2 the 8-wide tree, 3 the caller's tree verbatim; else what the
// render's closest-hit rays walk.  The one-ray-per-lane kernels keep the whole stack in LDS: a 4-wide tree deeper than 64 KB of stack falls back to the binary / verbatim walk
typedef void (*TraceKernel)(SceneView, int, int, const float*, const float*, const float*, const float*, int*, float*, int*, float*);
typedef void (*SurfaceKernel)(SceneView, TexView, int, int, const float*, const float*, const float*, const float*, int*, float*, float*, SampView);
typedef void (*SurfaceProcKernel)(SceneView, TexView, int, int, const float*, const float*, const float*, const float*, int*, float*, float*, SampView, ProcView);
struct TraceLaunch { TraceKernel trace; SurfaceKernel surface; size_t lds; int depth; int mode; };   // (surface: null for the 8-wide walk, which only trace_walk = 2 selects; mode: the kMode that runs, + 16 for the lean flat instance)
template <int M> TraceLaunch trace_row(size_t lds, int depth) { TraceLaunch t = { k_trace<M>, k_surface<M>, lds, depth, M }; return t; }
// the hooks that ride on k_trace's walk (k_light_pdf, k_shading_normal, k_shading_normal_mapped): f(integral_constant<int, kMode>) for the mode trace_kernel chose; null
// for the 8-wide walk (mode 3) and the lean flat instance, of which these hooks have no instance
template <class F> auto by_trace_mode(int mode, F f) -> decltype(f(std::integral_constant<int, 0>()))
{
	switch (mode)
	{
	case 0: return f(std::integral_constant<int, 0>());
	case 1: return f(std::integral_constant<int, 1>());
	case 2: return f(std::integral_constant<int, 2>());
	case 4: return f(std::integral_constant<int, 4>());
	case 5: return f(std::integral_constant<int, 5>());
	case 6: return f(std::integral_constant<int, 6>());
	default: return nullptr;
	}
}
TraceLaunch trace_kernel(const ScenePlan& p, int tw, bool generic = true)   // generic false (jp_trace without JpOptions::reserved[0] == 1): a scene of flat shapes gets the lean closest-hit walk
{
	const size_t q4lds = (size_t)p.stack_depth_q4 * JP_BLOCK * sizeof(int);
	if (p.trav_mode == 3 && tw == 2) { TraceLaunch t = { k_trace<3>, nullptr, p.lds_bytes_shadow, p.stack_depth, 3 }; return t; }
	if (p.trav_mode == 5 && p.cert && q4lds <= 64 * 1024 && tw != 3) return trace_row<6>(q4lds, p.stack_depth_q4);
	if (p.trav_mode == 5) return trace_row<5>(p.lds_bytes, p.stack_depth);
	if (p.use_q4 && q4lds <= 64 * 1024 && tw != 1) return trace_row<4>(q4lds, p.stack_depth_q4);
#ifndef JP_NO_EXTEND_POOL
	if (lean_traversal(p, generic) && p.sv.n_prims <= 32) { TraceLaunch t = { k_trace_pool, k_surface<2>, p.lds_bytes + pool_lds_bytes(), p.stack_depth, 2 + 16 }; return t; }   // (k_surface<2> takes less LDS than it is given)
#endif
	if (lean_traversal(p, generic)) { TraceLaunch t = { k_trace_flat, k_surface<2>, p.lds_bytes, p.stack_depth, 2 + 16 }; return t; }
	return p.trav_mode == 2 ? trace_row<2>(p.lds_bytes, p.stack_depth) : (p.trav_mode == 1 ? trace_row<1>(p.lds_bytes, p.stack_depth) : trace_row<0>(p.lds_bytes, p.stack_depth));
}

// jp_occluded: the any-hit twin of k_trace, one ray per lane.  tw == 0: the structure shadow_kernel gives the render's shadow rays (the lane refill kernels drive
// the same Walker steps); tw 1 / 2 / 3 as for trace_kernel, so that both hooks can be put on one structure.  Each row takes the grid and the LDS of k_trace's row
// for that mode; walk: the kMode that runs, + 16 for the lean flat instance (jp_occluded's walk_out)
typedef void (*OccludedKernel)(SceneView, int, int, const float*, const float*, const float*, const float*, int*);
struct OccludedLaunch { OccludedKernel occluded; size_t lds; int depth; int walk; };
template <int M> OccludedLaunch occluded_row(size_t lds, int depth) { OccludedLaunch t = { k_occluded<M>, lds, depth, M }; return t; }
OccludedLaunch occluded_kernel(const ScenePlan& p, int tw, bool generic)
{
	const size_t q4lds = (size_t)p.stack_depth_q4 * JP_BLOCK * sizeof(int);
	if (p.trav_mode == 3 && tw == 2) return occluded_row<3>(p.lds_bytes_shadow, p.stack_depth);
	if (p.trav_mode == 5 && p.cert && q4lds <= 64 * 1024 && tw != 3) return occluded_row<6>(q4lds, p.stack_depth_q4);
	if (p.trav_mode == 5) return occluded_row<5>(p.lds_bytes, p.stack_depth);
	if (p.q4_shadow && q4lds <= 64 * 1024 && tw != 1) return occluded_row<4>(q4lds, p.stack_depth_q4);
	if (p.trav_mode == 3 && tw != 1) return occluded_row<3>(p.lds_bytes_shadow, p.stack_depth);
	if (lean_traversal(p, generic)) { OccludedLaunch t = { k_occluded<2, FeatFlat>, p.lds_bytes, p.stack_depth, 2 + 16 }; return t; }
	return p.trav_mode == 2 ? occluded_row<2>(p.lds_bytes, p.stack_depth) : (p.trav_mode == 1 ? occluded_row<1>(p.lds_bytes, p.stack_depth) : occluded_row<0>(p.lds_bytes, p.stack_depth));
}

// The bounces of one batch, between ray generation and the resolve: per bounce k_extend, [k_texel, k_normal,] k_shade and k_shadow on the context's queue set, and
// the drain of null-material scenes.  The other two integrators trace their batch in k_other: no bounce.  One text for render_one and the adaptive driver
// (jp_adaptive.h), whose kernels between the list twins are these launches.
struct BounceLaunch { const ExtendLaunch& ek; const ShadowLaunch& sk; const ShadeLaunch& shade; bool tex, smooth; const TexView& tv; const MipView& mv_cone; const NormView& nv; int* d_spill; DevCounters* d_cnt; };
int launch_bounces(JpContext* c, const JpRenderParams* rp, const ScenePlan& p, const RenderConst& rc, int grid, const BounceLaunch& b)
{
	const ExtendLaunch& ek = b.ek; const ShadowLaunch& sk = b.sk; int* const d_spill = b.d_spill; DevCounters* const d_cnt = b.d_cnt;
	int cur = 0;
	int iters = rp->integrator != JP_INTEGRATOR_PATH ? 0 : rp->max_depth + 1;
	for (int it = 0;; it++)
	{
		if (it >= iters)
		{
			if (rp->integrator != JP_INTEGRATOR_PATH || !p.has_null_material || it > iters + 64) break;
			// null-material primitives re-queue a path without consuming a bounce (integrator.cc:349-353): ask the device
			DevCounters h; HIP_TRY(hipMemcpyAsync(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream));
			if (h.n_queue[cur] == 0) break;
		}
		{
			Stamper t(c, CLS_EXTEND);
			if (ek.refill) hipLaunchKernelGGL(ek.refill, dim3(grid), dim3(JP_BLOCK), ek.lds, c->stream, p.sv, c->q, cur, ek.words, d_spill, d_cnt);
			else hipLaunchKernelGGL(ek.plain, dim3(grid), dim3(JP_BLOCK), ek.lds, c->stream, p.sv, c->q, cur, ek.words, d_cnt);
		}
		{
			Stamper t(c, CLS_SHADE);
			if (b.tex) launch_texel(c, p, grid, cur, b.tv, b.mv_cone);         // textured scenes: k_texel leaves the texture's answer for every hit, the textured twin shades with it
			if (b.smooth) launch_normal(c, p, grid, cur, b.nv);                // scenes with vertex normals or normal maps: Ns for every hit it applies to, the smooth twin shades with it
			b.shade(c->stream, grid, p.shade_lds_bytes, p.sv, c->q, rc, cur, d_cnt);
		}
		HIP_TRY(hipGetLastError());                                       // a failed launch (k_extend / k_shade) is reported where it happens, not at the end of the frame
		if (it < rp->max_depth || p.has_null_material)                     // at bounce == maxDepth Li() breaks before the NEE (integrator.cc:340-343)
		{
			Stamper t(c, CLS_SHADOW);
			if (sk.cert_fell_back) c->cert_fell_back = true;                 // the one-ray-per-lane kernels walk the caller's tree verbatim
			if (sk.refill) hipLaunchKernelGGL(sk.refill, dim3(grid), dim3(JP_BLOCK), sk.lds, c->stream, p.sv, c->q, rc, sk.words, d_spill, d_cnt);
			else hipLaunchKernelGGL(sk.plain, dim3(grid), dim3(JP_BLOCK), sk.lds, c->stream, p.sv, c->q, rc, sk.words, d_cnt);
			HIP_TRY(hipGetLastError());
		}
		cur ^= 1;
	}
	return JP_OK;
}

int render_one(JpContext* c, const JpRenderParams* rp, float* film_dev, bool sync, int lane_index = 0, int lane_count = 1, int lane_group = 4, bool ev0_recorded = false)
{
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_render: no scene uploaded");
	const ScenePlan& p = c->plan; Shard sh; DevCounters* const d_cnt = c->cnt.get<DevCounters>();
	if (const int e = shard_of(rp, sh, lane_index, lane_count, lane_group); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const long long npix = (long long)sh.lane_rows * rp->width;

	if (!ev0_recorded) HIP_TRY(hipEventRecord(c->ev0, c->stream));          // (with several lanes render_impl records it before the first lane is enqueued)
	HIP_TRY(hipMemsetAsync(film_dev, 0, sizeof(float) * 3 * (size_t)rp->width * rp->height, c->stream));
	HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(DevCounters), c->stream));
	if (const int e = variance_begin(c, rp, npix); e != JP_OK) return e;
	c->evused = 0; c->stamps.clear();
	unsigned long long samples = 0;
	if (npix > 0)
	{
		if (npix > (1 << 24)) return fail(JP_ERR_UNSUPPORTED, "jp_render: more than 2^24 pixels per shard");
		// a shadow entry's header packs (slot, ray count) in 32 bits: 27 + 5 as a rule; batches of up to 2^26 slots (regions of <= 8192
		// slots: up to 8192 workgroups a launch, whose tail -- the last workgroups finishing on an emptying GPU -- weighs a quarter of
		// what it does with 2^24)
		const int slot_bits = p.n_planes <= 31 ? 27 : 24;
		const unsigned int PMAX = slot_bits == 27 ? (1u << 26) : (1u << 24);
		// memory budget for the queues: ~ (136 + 32 * planes) bytes per slot.  ONE budget -- half of what is free, at most 24 GB per lane --
		// shared by the lanes that render concurrently (each lane sizes its own queue set from its share), and when the allocation still
		// fails (another process took the memory in between) the batch is halved and tried again before the call gives up
		size_t freeB = 0, totalB = 0; hipMemGetInfo(&freeB, &totalB);
		const bool smooth = p.smooth && rp->integrator == JP_INTEGRATOR_PATH;    // vertex normals: k_normal + k_shade_smooth* (the debug integrator ignores them)
		const size_t per = 136 + 32 * (size_t)p.n_planes + (smooth ? 16 : 0);
		size_t budget = std::min<size_t>((size_t)24 << 30, (freeB / (size_t)std::max(1, lane_count) + (c->cap ? (size_t)c->cap * (136 + 32 * (size_t)c->planes_alloc) : 0)) / 2);
		if (c->opt.max_slots > 0) budget = std::min<size_t>(budget, (size_t)c->opt.max_slots * per);
		int sbatch = 1; unsigned int P = 0, G = 1, R = JP_BLOCK, cap = 0;
		for (int attempt = 0;; attempt++)
		{
			const unsigned int pcap = (unsigned int)std::min<size_t>(PMAX, std::max<size_t>((size_t)npix, budget / per));
			sbatch = (int)std::max<long long>(1, std::min<long long>(rp->spp, pcap / npix));
			{   // equal batches: ceil(spp / sbatch) batches of (nearly) the same size instead of full ones and a remainder (1024 spp in batches of
				// 192 would end with a 64-spp batch whose launches fill a third of the GPU)
				const int nb = (rp->spp + sbatch - 1) / sbatch;
				sbatch = (rp->spp + nb - 1) / nb;
			}
			if ((long long)sbatch * npix > (long long)PMAX) return fail(JP_ERR_UNSUPPORTED, "jp_render: shard too large for one batch");
			P = (unsigned int)((long long)sbatch * npix);
			const unsigned int nchunks = (P + JP_BLOCK - 1) / JP_BLOCK;
			G = std::max(1u, std::min(nchunks, (unsigned int)(c->n_cus * c->blocks_per_cu)));   // one region per workgroup
			G = std::max(G, (nchunks + JP_SHADE_TILE / JP_BLOCK - 1) / (JP_SHADE_TILE / JP_BLOCK));   // R <= JP_SHADE_TILE: k_shade partitions a whole region in LDS and counts its fills in 16 bits
			R = ((nchunks + G - 1) / G) * JP_BLOCK;
			cap = G * R;
			const int st = ensure_queues(c, cap, p.n_planes, G);
			if (st == JP_OK) break;
			if (sbatch <= 1 || attempt >= 6) return st;                 // one sample per pixel does not fit either: out of device memory
			budget = (size_t)sbatch / 2 * (size_t)npix * per;              // half the batch
		}
		c->q.cap = cap; c->q.R = R;
		const bool tex = p.textured && rp->integrator == JP_INTEGRATOR_PATH;
		// the side words of k_texel: one per queue position, allocated for textured scenes only
		if (tex) if (const int e = reserve_idle(c, c->side, (size_t)cap * sizeof(unsigned int)); e != JP_OK) return e;
		TexView tv = p.tv; tv.side = c->side.get<unsigned int>();
		MipView mv_cone = {};                                         // mip maps (jp_mipmap.h): k_texel_m / k_texel_p and the cones of this queue set, allocated for scenes with a pyramid or an antialiased procedural only
		if (tex && (p.mip_on > 0 || p.proc_aa > 0)) { mv_cone = p.mv; if (const int e = ensure_cone(c, cap, mv_cone); e != JP_OK) return e; }
		// JP_ESTIMATOR_MIS (render_impl refused a scene without the light table): the side records of this queue set
		const bool mis = c->estimator == JP_ESTIMATOR_MIS && rp->integrator == JP_INTEGRATOR_PATH;
		MisView mv = {};
		if (mis) if (const int e = ensure_mis_side(c, cap, mv); e != JP_OK) return e;
		NormView nv = p.nv;
		if (smooth) if (const int e = ensure_normal_side(c, cap, nv); e != JP_OK) return e;
		if (const int e = reserve_idle(c, c->spill, spill_need(p, p.persist ? deepest_walk(p) : 0, G) * sizeof(int)); e != JP_OK) return e;
		if (const int e = reserve_idle(c, c->pix_acc, (size_t)npix * 16); e != JP_OK) return e;
		int* const d_spill = c->spill.get<int>(); float4* const d_pix_acc = c->pix_acc.get<float4>();

		RenderConst rc; rc.width = rp->width; rc.height = rp->height; rc.spp = rp->spp; rc.max_depth = rp->max_depth; rc.seed = rp->seed;
		rc.band_rows = sh.band; rc.shard_index = sh.index; rc.shard_count = sh.count; rc.npix = (int)npix; rc.local_rows = sh.lane_rows; rc.n_planes = p.n_planes;
		rc.lane_index = lane_index; rc.lane_count = lane_count; rc.lane_rows = lane_group; rc.class_mask = p.class_mask; rc.sampler_debug = rp->sampler_mode == JP_SAMPLER_DEBUG ? 1 : 0;
		// measured: +6 % on the 280k-triangle scene (cache reuse), -8 % on the LDS-resident Cornell box (coherent waves finish
		// together or not at all, which unbalances the workgroups) -> tiles only when traversal goes through global memory
		rc.slot_bits = slot_bits;
		rc.tiled = 0;                                                  // (16 x 4 pixel tiles per wave: measured slower with the wide trees and with the LDS-resident box, profiles/r03e_compact_regions_ab.txt; the fused schedule keeps them)
		// compact regions (k_raygen): scenes walked through global memory -- one lane on the 280k-triangle scene: k_extend 64.1 -> 55.8 ms,
		// k_shadow 47.1 -> 40.5 ms per 512 spp (the workgroups in flight share an image area, hence tree nodes: L2), three lanes +1.2 %;
		// films bit-identical.  JETPBRT_COMPACT_REGIONS=0 / 1 forces it.
		rc.compact = (p.trav_mode != 2 && p.trav_mode != 1 && npix % JP_BLOCK == 0) ? 1 : 0;
		if (c->opt.compact_regions != 0) rc.compact = (c->opt.compact_regions > 0 && npix % JP_BLOCK == 0) ? 1 : 0;
		const int grid = (int)G;
		const bool generic = c->opt.reserved[0] == 1;                // JpOptions::reserved[0]: the kernels with every feature in them, whatever the scene holds
		const ExtendLaunch ek = extend_kernel(p, generic); const ShadowLaunch sk = shadow_kernel(p, R, generic); const OtherKernel ok = other_kernel(p);
		const ShadeLaunch shade = shade_launch(shade_choice(p, tex, mis, smooth, generic), ShadeViews(tv, p.pv, p.ev, mv, nv));
		JpLensPlan lp;                                                 // jp_set_lens: k_raygen<true> / k_other form the lens ray; the bounces never know
		if (const int e = lens_plan_of(c, lp); e != JP_OK) return e;
		JpProjectionPlan pp;                                           // jp_set_projection: k_raygen_proj / k_other form the projected ray; its cone spread goes to k_texel_m / k_texel_p
		if (const int e = proj_plan_of(c, pp); e != JP_OK) return e;
		if (c->proj_on) mv_cone.gamma0 = pp.gamma0;
		for (int s0 = 0; s0 < rp->spp; s0 += sbatch)
		{
			rc.s0 = s0; rc.sbatch = std::min(sbatch, rp->spp - s0);
			{
				Stamper t(c, CLS_OTHER);
				if (c->proj_on) hipLaunchKernelGGL(k_raygen_proj, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, pp);
				else if (c->lens_on) hipLaunchKernelGGL(k_raygen<true>, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, lp);
				else hipLaunchKernelGGL(k_raygen<false>, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, NoLens());
			}
			if (rp->integrator != JP_INTEGRATOR_PATH)
			{   // the other two integrators: one megakernel launch per batch (k_other), then the same per-pixel sum
				Stamper t(c, CLS_OTHER);
				const int ogrid = (int)std::min<unsigned int>((P + JP_BLOCK - 1) / JP_BLOCK, (unsigned int)(c->n_cus * 16));
				hipLaunchKernelGGL(ok, dim3(ogrid), dim3(JP_BLOCK), p.lds_bytes, c->stream, p.sv, c->q, rc, rp->integrator, p.stack_depth, d_cnt, c->lens_on ? 1 : 0, lp, pp);
			}
			if (const int e = launch_bounces(c, rp, p, rc, grid, BounceLaunch{ ek, sk, shade, tex, smooth, tv, mv_cone, nv, d_spill, d_cnt }); e != JP_OK) return e;
			{ Stamper t(c, CLS_OTHER); launch_resolve(c, c->q, rc, npix, d_pix_acc, film_dev, s0 == 0 ? 1 : 0, s0 + rc.sbatch >= rp->spp ? 1 : 0); }
			samples += (unsigned long long)rc.sbatch * (unsigned long long)npix;
		}
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipEventRecord(c->ev1, c->stream));
	c->own_samples = samples;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

// ---- stream lanes: the shard's bands dealt to L lanes, rendered concurrently on L streams with L queue sets ---------------
__global__ void __launch_bounds__(JP_BLOCK) k_add_film(float* __restrict__ dst, const float* __restrict__ src, size_t n)
{
	// the lanes' films are disjoint (zero outside a lane's bands), so the sum is the union, bit for bit
	for (size_t i = (size_t)blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * JP_BLOCK) dst[i] += src[i];
}

int make_lanes(JpContext* c, int extra)
{
	if (!c->ev_added && hipEventCreateWithFlags(&c->ev_added, hipEventDisableTiming) != hipSuccess) return fail(JP_ERR_DEVICE, "jp_render: event allocation failed");
	while ((int)c->lanes.size() < extra)
	{
		JpContext* l = new JpContext;
		l->device = c->device; l->is_lane = true; l->n_cus = c->n_cus; l->blocks_per_cu = c->blocks_per_cu; l->opt = c->opt; l->opt_env = c->opt_env;
		std::memset(&l->counters, 0, sizeof(l->counters)); std::memset(&l->q, 0, sizeof(l->q));
		if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&l->ev0) != hipSuccess || hipEventCreate(&l->ev1) != hipSuccess
		    || l->cnt.reserve(sizeof(DevCounters)) != hipSuccess)
		{ jp_destroy_context(l); return fail(JP_ERR_DEVICE, "jp_render: stream/event allocation for an extra lane failed"); }
		c->lanes.push_back(l);
	}
	return JP_OK;
}

// a lane walks the same device tables as its parent (it owns none of them): the plan, plus what really is per lane
void sync_lane_scene(JpContext* c, JpContext* l)
{
	l->plan = c->plan;                                               // (the lane's side array is its own, allocated with its queues)
	if (!l->plan.textured && l->side) { hipStreamSynchronize(l->stream); l->side.reset(); }   // untextured scene: not kept
	if (l->plan.mip_on == 0 && l->plan.proc_aa == 0 && l->cone) { hipStreamSynchronize(l->stream); l->cone.reset(); }   // (and the cones of k_texel_m)
	if (!l->plan.smooth && l->nside) { hipStreamSynchronize(l->stream); l->nside.reset(); }   // (the same for the side records of k_normal)
	l->profiling = c->profiling; l->opt = c->opt;                    // render_one(lane) reads max_slots / compact_regions from its own context
	l->estimator = c->estimator;                                     // ... and the estimator (its side records are its own, like its queues)
	l->lens = c->lens; l->lens_on = c->lens_on;                      // ... and the lens
	l->proj = c->proj; l->proj_on = c->proj_on;                      // ... and the projection
	l->film_state = c->film_state; l->film_on = c->film_on;          // ... and the film state (a lane resolves its own bands)
	l->var_on = c->var_on;                                           // ... and whether it keeps the moments (render_impl gives it a variance plane of its own)
}

// ---- fused schedule: one k_path launch per batch (jp_path.h) --------------------------------------------------------------
// OPT-IN (JETPBRT_FUSED=1; FScene / CLI: --fused).  Measured in round 3 (profiles/r03a_fused_ab.txt): films bit-identical to the
// per-bounce launches, queue memory 1.2 GB instead of 13-40 GB -- and 20 % (Cornell) to 57 % (280k-triangle scene) SLOWER than three
// stream lanes: k_path inherits k_shade's 168 registers, so the traversal phases run at 3 waves per SIMD instead of 8, and a region that
// fits LDS-resident hit records and radiance (1024 paths) gives every phase of a late bounce less than one path per thread.
// Which scenes: the path integrator on scenes whose tables fit LDS with <= 4 emitting lights (every scene of the reference),
// traversal modes 2 (flat leaf list), 0 / 3 (binary + 8-wide trees, walkers) and 5 (reference semantics).  Mode 1 (a small tree
// staged into LDS next to its stack) and larger tables keep the per-bounce launches.
bool fused_eligible(const JpContext* c, const JpRenderParams* rp)
{
	if (c->opt.fused <= 0) return false;                             // JpOptions::fused
	if (c->is_lane || !c->plan.have_scene || rp->integrator != JP_INTEGRATOR_PATH) return false;
	if (!c->plan.tables_in_lds || c->plan.n_planes > 4) return false;          // (its own LDS budget: render_fused shrinks the region until the layout fits)
	if (c->plan.cert) return false;                                       // the certified walk lives in the per-bounce traversal kernels
	if (c->plan.textured) return false;                                   // textures: k_texel + k_shade_tex live in the per-bounce launches
	if (c->plan.pick) return false;                                       // JP_LIGHTS_POWER_ONE: k_shade_pick lives there too
	if (c->plan.smooth) return false;                                     // vertex normals: k_normal + k_shade_smooth* as well
	if (c->lens_on) return false;                                         // a lens: k_raygen<true> lives in the per-bounce launches (k_path forms the pinhole ray)
	if (c->proj_on) return false;                                         // a projection: k_raygen_proj likewise
	if (c->plan.trav_mode == 2) return c->plan.shade_prims_in_lds;
	return c->plan.trav_mode == 0 || c->plan.trav_mode == 3 || c->plan.trav_mode == 5;
}

typedef void (*PathKernel)(SceneView, Queues, RenderConst, PathConst, int*, DevCounters*);
PathKernel path_kernel(const ScenePlan& p)
{
	const bool so = p.shade_sort;
	switch (p.trav_mode)
	{
	case 2: return so ? k_path<2, 2, true, true, true> : k_path<2, 2, true, false, true>;
	case 3:
		if (p.use_q4) return p.q4_shadow ? (so ? k_path<4, 4, false, true, true> : k_path<4, 4, false, false, true>) : (so ? k_path<4, 3, false, true, true> : k_path<4, 3, false, false, true>);
		return so ? k_path<0, 3, false, true, true> : k_path<0, 3, false, false, true>;
	case 5: return so ? k_path<5, 5, false, true, false> : k_path<5, 5, false, false, false>;
	default:
		if (p.use_q4) return so ? k_path<4, 4, false, true, true> : k_path<4, 4, false, false, true>;
		return so ? k_path<0, 0, false, true, true> : k_path<0, 0, false, false, true>;
	}
}

int render_fused(JpContext* c, const JpRenderParams* rp, float* film_dev, bool sync)
{
	const ScenePlan& p = c->plan; Shard sh; DevCounters* const d_cnt = c->cnt.get<DevCounters>();
	if (const int e = shard_of(rp, sh); e != JP_OK) return e;         // (fused_eligible: the path integrator, so the integrator checks cannot fire)
	HIP_TRY(hipSetDevice(c->device));
	const long long npix = (long long)sh.local_rows * rp->width;

	HIP_TRY(hipEventRecord(c->ev0, c->stream));
	HIP_TRY(hipMemsetAsync(film_dev, 0, sizeof(float) * 3 * (size_t)rp->width * rp->height, c->stream));
	HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(DevCounters), c->stream));
	if (const int e = variance_begin(c, rp, npix); e != JP_OK) return e;
	c->evused = 0; c->stamps.clear();
	unsigned long long samples = 0;
	c->last_fused = 1; c->last_lanes = 1;
	if (npix > 0)
	{
		if (npix > (1 << 24)) return fail(JP_ERR_UNSUPPORTED, "jp_render: more than 2^24 pixels per shard");
		const PathKernel kern = path_kernel(p);
		const bool flat = p.trav_mode == 2;
		const int modeE = flat ? 2 : (p.trav_mode == 5 ? 5 : 0);
		// ---- batch: the radiance array holds one float4 per path of the batch (the only per-path array that outlives a job) ----
		size_t freeB = 0, totalB = 0; hipMemGetInfo(&freeB, &totalB);
		size_t budget = std::min<size_t>((size_t)4 << 30, (freeB + c->fqb.lacc.bytes()) / 4);
		if (c->opt.max_slots > 0) budget = std::min<size_t>(budget, (size_t)c->opt.max_slots * 16);
		const size_t PMAX = (size_t)1 << 26;
		const size_t pcap = std::min<size_t>(PMAX, std::max<size_t>((size_t)npix, budget / 16));
		int sbatch = (int)std::max<long long>(1, std::min<long long>(rp->spp, (long long)(pcap / (size_t)npix)));
		{ const int nb = (rp->spp + sbatch - 1) / sbatch; sbatch = (rp->spp + nb - 1) / nb; }       // equal batches
		// ---- job shape: R paths = PG pixels x S samples.  A wave's 64 lanes are 64 neighbouring pixels of one sample. ----
		unsigned int R = 1024;
		{ const int v = c->opt.fused_region; if (v >= JP_BLOCK && v <= 8192) R = (unsigned int)(v / JP_BLOCK) * JP_BLOCK; }
		int S = 16;
		{ const int v = c->opt.fused_job_spp; if (v >= 1 && v <= 128) S = v; }
		const int n_tab = 2 * p.sv.n_lights + 4 * p.sv.n_mats + (p.sv.n_mats + 3) / 4, n_tab_all = n_tab + (flat ? 8 * p.sv.n_prims : 0);
		const int deepE = extend_depth(p), deepS = shadow_depth(p);
		const int ecap = flat ? 0 : std::min(deepE, p.stack_lds_words), scap = flat ? 0 : std::min(deepS, p.stack_lds_words);
		PathLds L = path_lds_layout(modeE, n_tab_all, p.sv.n_prims, R, p.n_planes, ecap, scap, p.shade_sort);
		while (L.total > 64 * 1024 && R > JP_BLOCK) { R -= JP_BLOCK; L = path_lds_layout(modeE, n_tab_all, p.sv.n_prims, R, p.n_planes, ecap, scap, p.shade_sort); }
		if (L.total > 64 * 1024) return fail(JP_ERR_UNSUPPORTED, "jp_render: the fused schedule's LDS layout does not fit this scene (JETPBRT_FUSED=0 selects the per-bounce launches)");
		S = std::max(1, std::min(S, std::min(sbatch, (int)(R / 64))));
		int PG = (int)(R / (unsigned int)S); if (PG >= 64) PG &= ~63;
		if ((long long)PG > npix) PG = (int)npix;
		const int npg = (int)((npix + PG - 1) / PG), nsb = (sbatch + S - 1) / S;
		const unsigned long long njobs = (unsigned long long)npg * nsb;
		if (njobs >= (1ull << 32)) return fail(JP_ERR_UNSUPPORTED, "jp_render: too many jobs per batch");
		// ---- resident workgroups: as many as the kernel's registers and LDS allow, persistent, taking jobs from a counter ----
		HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total));
		int per_cu = 0;
		HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kern, JP_BLOCK, L.total));
		per_cu = std::max(1, per_cu);
		{ const int v = c->opt.fused_workgroups; if (v >= 1 && v <= 16) per_cu = v; }
		const unsigned int G = (unsigned int)std::min<unsigned long long>(njobs, (unsigned long long)c->n_cus * per_cu);
		const unsigned int cap = G * R;
		if (c->fcap < cap || c->fplanes < p.n_planes)
		{
			HIP_TRY(hipStreamSynchronize(c->stream));
			const unsigned int ncap = std::max(cap, c->fcap); const int npl = std::max(p.n_planes, c->fplanes);
			QueueBufs& qb = c->fqb; Queues& q = c->fq;
			{ DevBuf lacc = std::move(qb.lacc); qb = QueueBufs(); qb.lacc = std::move(lacc); }   // all or nothing, except the radiance array: it is sized by the batch (below) and stays
			c->fcap = 0; c->fplanes = 0; q = Queues();
			auto alloc = [](DevBuf& b, auto*& p, size_t bytes) { return reserve(b, p, bytes) == hipSuccess; };
			bool ok = true;
			for (int b = 0; b < 2 && ok; b++) ok = alloc(qb.ray_o[b], q.ray_o[b], (size_t)ncap * 16) && alloc(qb.ray_d[b], q.ray_d[b], (size_t)ncap * 16) && alloc(qb.beta[b], q.beta[b], (size_t)ncap * 16);
			ok = ok && alloc(qb.sh_o, q.sh_o, (size_t)ncap * 16) && alloc(qb.sh_d, q.sh_d, (size_t)ncap * 16 * npl) && alloc(qb.sh_c, q.sh_c, (size_t)ncap * 16 * npl);
			if (!ok) { qb = QueueBufs(); return fail(JP_ERR_DEVICE, "jp_render: out of device memory for the region queues"); }
			c->fcap = ncap; c->fplanes = npl;
		}
		const size_t P = (size_t)sbatch * (size_t)npix;
		if (const int e = reserve_idle(c, c->fqb.lacc, P * 16); e != JP_OK) return e;      // the batch's radiance array
		c->fq.lacc = c->fqb.lacc.get<float4>(); c->fq.cap = c->fcap; c->fq.R = R;
		const int nbatches = (rp->spp + sbatch - 1) / sbatch;
		if (const int e = reserve_idle(c, c->jobs, (size_t)nbatches * 4); e != JP_OK) return e;
		unsigned int* const d_jobs = c->jobs.get<unsigned int>();
		HIP_TRY(hipMemsetAsync(d_jobs, 0, (size_t)nbatches * 4, c->stream));
		if (const int e = reserve_idle(c, c->spill, spill_need(p, flat ? 0 : std::max(deepE, deepS), G) * sizeof(int)); e != JP_OK) return e;
		if (const int e = reserve_idle(c, c->pix_acc, (size_t)npix * 16); e != JP_OK) return e;
		int* const d_spill = c->spill.get<int>(); float4* const d_pix_acc = c->pix_acc.get<float4>();

		RenderConst rc; std::memset(&rc, 0, sizeof(rc));
		rc.width = rp->width; rc.height = rp->height; rc.spp = rp->spp; rc.max_depth = rp->max_depth; rc.seed = rp->seed;
		rc.band_rows = sh.band; rc.shard_index = sh.index; rc.shard_count = sh.count; rc.npix = (int)npix; rc.local_rows = sh.local_rows; rc.n_planes = p.n_planes;
		rc.lane_index = 0; rc.lane_count = 1; rc.lane_rows = 4; rc.class_mask = p.class_mask; rc.sampler_debug = rp->sampler_mode == JP_SAMPLER_DEBUG ? 1 : 0;
		rc.slot_bits = JP_PATH_LI_BITS;
		// 16 x 4 pixel tiles: a job's 64-pixel groups are patches of the image, so the lanes of a wave start as neighbours (camera
		// rays and first shadow rays of large scenes share nodes).  JETPBRT_NO_TILES=1: row-major groups.
		rc.tiled = (rp->width % 16 == 0 && sh.local_rows % 4 == 0 && PG % 64 == 0 && p.trav_mode != 2) ? 1 : 0;
		PathConst pc; pc.R = R; pc.PG = PG; pc.S = S; pc.npg = npg; pc.nsb = nsb; pc.ecap = ecap; pc.scap = scap;
		pc.max_iters = rp->max_depth + 1 + (p.has_null_material ? 64 : 0);
		c->last_region = (int)R; c->last_wgs = (int)G;
		for (int s0 = 0, bi = 0; s0 < rp->spp; s0 += sbatch, bi++)
		{
			rc.s0 = s0; rc.sbatch = std::min(sbatch, rp->spp - s0);
			pc.nsb = (rc.sbatch + S - 1) / S; pc.job = d_jobs + bi;
			const unsigned int g = (unsigned int)std::min<unsigned long long>((unsigned long long)npg * pc.nsb, (unsigned long long)G);
			{ Stamper t(c, CLS_PATH); hipLaunchKernelGGL(kern, dim3(g), dim3(JP_BLOCK), L.total, c->stream, p.sv, c->fq, rc, pc, d_spill, d_cnt); }
			HIP_TRY(hipGetLastError());
			{ Stamper t(c, CLS_OTHER); launch_resolve(c, c->fq, rc, npix, d_pix_acc, film_dev, s0 == 0 ? 1 : 0, s0 + rc.sbatch >= rp->spp ? 1 : 0); }
			HIP_TRY(hipGetLastError());
			samples += (unsigned long long)rc.sbatch * (unsigned long long)npix;
		}
	}
	HIP_TRY(hipEventRecord(c->ev1, c->stream));
	c->own_samples = samples;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int render_impl(JpContext* c, const JpRenderParams* rp, float* film_dev, bool sync)
{
	if (!c || !rp || !film_dev) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: null argument");
	c->last_hdr = 0;
	c->last_var = c->var_on ? 1 : 0;
	c->ad_info.adaptive_last_render = 0;                                  // (jp_adaptive.h's driver does not come through here)
	if (!c->var_on && (c->var_mom || (!c->lanes.empty() && c->lanes[0]->var_mom))) { c->var_mom.reset(); for (JpContext* l : c->lanes) l->var_mom.reset(); }   // (left by a variance render that did not wait for its stream)
	c->last_lanes = 1; c->last_fused = 0; c->last_textured = 0; c->last_picked = 0; c->last_mapped = 0; c->last_mis = 0; c->last_smooth = 0; c->last_lens = 0; c->last_proj = 0; c->last_proj_gamma0 = 0.f; c->last_nmapped = 0; c->last_sampled = 0; c->last_mip = 0; c->last_proc = 0;
	if (c->plan.mapped && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator shades with the geometric normal (scene uploaded with normal maps, jp_set_normal_maps)");
	if (c->plan.smooth && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator shades with the geometric normal (scene uploaded with vertex normals, jp_set_vertex_normals)");
	if (c->plan.env && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator does not sample environment maps (jp_set_environment_map)");
	if (c->plan.pick && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator samples every light (scene uploaded with JP_LIGHTS_POWER_ONE)");
	if (c->plan.textured && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator does not sample textures (scene uploaded by jp_upload_scene_textured)");
	if (c->estimator == JP_ESTIMATOR_MIS && rp->integrator == JP_INTEGRATOR_WHITTED) return fail(JP_ERR_UNSUPPORTED, "jp_render: the Whitted integrator has one estimator (jp_set_estimator: JP_ESTIMATOR_MIS is the path integrator's)");
	if (c->estimator == JP_ESTIMATOR_MIS && rp->integrator == JP_INTEGRATOR_PATH && c->plan.have_scene && !c->plan.pick)
		return fail(JP_ERR_UNSUPPORTED, "jp_render: JP_ESTIMATOR_MIS needs a scene uploaded with JP_LIGHTS_POWER_ONE (jp_set_light_sampling): the light strategy's pdf comes from the light table");
	if (c->proj_on && c->plan.have_scene)
	{   // jp_set_projection: refused here, before any lane starts (a lens together with a projection; a camera the projection cannot stand on)
		JpProjectionPlan pp;
		if (const int e = proj_plan_of(c, pp); e != JP_OK) return e;
		c->last_proj = 1; c->last_proj_gamma0 = pp.gamma0;                // (every integrator forms the projected ray)
	}
	if (fused_eligible(c, rp)) return render_fused(c, rp, film_dev, sync);
	c->last_textured = c->plan.textured && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_picked = c->plan.pick && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_mapped = c->plan.env && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_mis = c->estimator == JP_ESTIMATOR_MIS && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_smooth = c->plan.smooth && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_nmapped = c->plan.mapped && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_sampled = ((c->plan.textured && c->plan.sm.tex) || (c->plan.mapped && c->plan.sm.map)) && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_mip = c->plan.textured && c->plan.mip_on > 0 && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_proc = c->plan.textured && c->plan.proc_on > 0 && rp->integrator == JP_INTEGRATOR_PATH ? 1 : 0;
	c->last_lens = c->lens_on ? 1 : 0;                                    // (every integrator forms the lens ray)
	// lanes: the shard's rows in groups of 4 dealt round-robin to L contexts.  Default: 3 lanes when each gets >= 16 groups and
	// full-size batches, else 2, else 1 (measured on the benchmark frame: 1 lane 2.19, 2 lanes 2.70, 3 lanes 2.82, 4 lanes 2.38
	// Gsamples/s).  JETPBRT_LANES = 1 .. 4 forces a count, JETPBRT_LANE_ROWS the group height.
	int forcedL = 0, group = 4;
	if (c->opt.lanes >= 1 && c->opt.lanes <= 4) forcedL = c->opt.lanes;
	if (c->opt.lane_rows >= 1 && c->opt.lane_rows <= 64) group = c->opt.lane_rows;
	int L = 1; Shard sh;
	if (!c->is_lane && c->plan.have_scene && !c->plan.has_null_material && rp->integrator == JP_INTEGRATOR_PATH && shard_of(rp, sh) == JP_OK)   // (bad parameters: render_one reports them)
	{
		const long long rows = sh.local_rows, groups = (rows + group - 1) / group;
		if (forcedL) L = (int)std::min<long long>(forcedL, std::max<long long>(1, groups));
		else
		{
			// worth it only when each lane still gets full-size batches (2^24 slots): measured -7 % at 512 x 512 x 64 spp
			// (half-size batches), +17 % / +24 % at 1024 spp with two / three lanes
			const long long samples = rows * rp->width * (long long)rp->spp;
			// round 2, measured on one rank's share of an 8- / 4-GPU frame (64 / 128 rows of 512 x 512, tools/gpu_shard_lanes.py): three lanes
			// beat two there as well (1/8 shard at 1024 spp 13.5 vs 14.8 ms, at 8192 spp 2570 vs 2334 Msamples/s), so the lane count follows
			// the sample count alone
			if (groups >= 3 && samples >= (2ll << 24)) L = 3;
			else if (groups >= 2 && samples >= (2ll << 24)) L = 2;
		}
	}
	if (L <= 1) return render_one(c, rp, film_dev, sync);

	HIP_TRY(hipSetDevice(c->device));
	int st = make_lanes(c, L - 1); if (st != JP_OK) return st;
	const size_t n = (size_t)rp->width * rp->height * 3;
	// workgroups per CU and lane (measured on the benchmark frame, two lanes: 2.51 Gsamples/s at 16 + 16, 2.70 at 8 + 8,
	// 2.74 at 6 + 6, 2.60 at 4 + 4; three lanes: 2.83 at 5 + 5 + 5; a single lane is best at 16)
	HIP_TRY(hipEventRecord(c->ev0, c->stream));                                       // render_ms starts before the first lane's kernels are enqueued
	const int bpc_single = c->blocks_per_cu, bpc_lane = c->bpc_from_env ? c->blocks_per_cu : std::max(4, 16 / L);
	for (int k = 1; k < L && st == JP_OK; k++)
	{
		JpContext* l = c->lanes[k - 1];
		sync_lane_scene(c, l);
		if (l->film.bytes() < n * sizeof(float)) c->added_valid = false;
		if (const int e = reserve_idle(c, l->film, n * sizeof(float)); e != JP_OK) return e;   // (waits for the PARENT's stream: its merge of the previous frame reads the lane film)
		if (c->var_on) { if (const int e = reserve_idle(c, l->var_plane, n / 3 * sizeof(float)); e != JP_OK) return e; l->var_dev = l->var_plane.get<float>(); }   // (likewise the lane's variance plane)
		if (c->added_valid) HIP_TRY(hipStreamWaitEvent(l->stream, c->ev_added, 0));   // the previous frame's merge still reads the lane film
		l->blocks_per_cu = bpc_lane;
		st = render_one(l, rp, l->film.get<float>(), false, k, L, group);
	}
	if (st == JP_OK) { c->blocks_per_cu = bpc_lane; st = render_one(c, rp, film_dev, false, 0, L, group, true); c->blocks_per_cu = bpc_single; }
	if (st != JP_OK) return st;
	for (int k = 1; k < L; k++)
	{
		JpContext* l = c->lanes[k - 1];
		HIP_TRY(hipStreamWaitEvent(c->stream, l->ev1, 0));                           // recorded at the end of the lane's render_one
		hipLaunchKernelGGL(k_add_film, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream, film_dev, l->film.get<const float>(), n);
		if (c->var_on) hipLaunchKernelGGL(k_add_film, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (n / 3 + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream, c->var_dev, l->var_plane.get<const float>(), n / 3);   // the variance planes are disjoint like the films
	}
	HIP_TRY(hipEventRecord(c->ev_added, c->stream)); c->added_valid = true;
	HIP_TRY(hipEventRecord(c->ev1, c->stream));                                       // render_ms: all lanes and the merge
	c->last_lanes = L;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int finish_one(JpContext* c, JpCounters& o)
{
	HIP_TRY(hipStreamSynchronize(c->stream));
	DevCounters h; HIP_TRY(hipMemcpy(&h, c->cnt.get<void>(), sizeof(h), hipMemcpyDeviceToHost));
	c->normal_ms = 0.0; c->normal_map_ms = 0.0; c->texel_ms = 0.0;
	o.closest_rays += h.closest; o.closest_hits += h.closest_hit; o.shadow_rays += h.shadow; o.shadow_occluded += h.shadow_occ; o.certified_fallback_rays += h.cert_fallback;
	for (const JpContext::Stamp& s : c->stamps)
	{
		float t = 0.f; if (hipEventElapsedTime(&t, c->evpool[s.a], c->evpool[s.b]) != hipSuccess) continue;
		if (s.cls == CLS_EXTEND) { o.extend_ms += t; o.extend_launches++; }
		else if (s.cls == CLS_SHADE) { o.shade_ms += t; o.shade_launches++; }
		else if (s.cls == CLS_SHADOW) { o.shadow_ms += t; o.shadow_launches++; }
		else if (s.cls == CLS_PATH) { o.path_ms += t; o.path_launches++; }
		else if (s.cls == CLS_NORMAL) c->normal_ms += t;
		else if (s.cls == CLS_NMAP) c->normal_map_ms += t;
		else if (s.cls == CLS_TEXEL) c->texel_ms += t;
		else o.other_ms += t;
	}
	return JP_OK;
}

int finish_counters(JpContext* c)
{
	HIP_TRY(hipSetDevice(c->device));
	JpCounters& o = c->counters;
	unsigned long long samples = c->own_samples;
	std::memset(&o, 0, sizeof(o));
	int st = finish_one(c, o); if (st != JP_OK) return st;
	for (int k = 1; k < c->last_lanes; k++)                                           // per-class times add up over the (overlapping) lanes
	{ samples += c->lanes[k - 1]->own_samples; st = finish_one(c->lanes[k - 1], o); if (st != JP_OK) return st; }
	float ms = 0.f; if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) ms = 0.f;
	o.render_ms = ms; o.samples = samples;
	return JP_OK;
}
}

extern "C" {

int jp_render_device(JpContext* c, const JpRenderParams* rp, void* film_rgb_device, int sync) { return render_impl(c, rp, (float*)film_rgb_device, sync != 0); }

int jp_render(JpContext* c, const JpRenderParams* rp, float* film_host)
{
	if (!c || !rp || !film_host) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: null argument");
	if (rp->width <= 0 || rp->height <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render: bad width/height");
	HIP_TRY(hipSetDevice(c->device));
	size_t n = (size_t)rp->width * rp->height * 3;
	if (const int e = ensure_film(c, n); e != JP_OK) return e;
	float* const d_film = c->film.get<float>();
	float* stage = c->h_film.reserve(n * sizeof(float)) == hipSuccess ? c->h_film.get<float>() : film_host;   // (no pinned memory: the pageable copy)
	int st = render_impl(c, rp, d_film, false); if (st != JP_OK) return st;
	HIP_TRY(hipMemcpyAsync(stage, d_film, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (stage != film_host) std::memcpy(film_host, stage, n * sizeof(float));
	return JP_OK;
}

int jp_render_rgb8(JpContext* c, const JpRenderParams* rp, uint8_t* rgb8_host, float* film_host)
{
	if (!c || !rp || !rgb8_host) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_rgb8: null argument");
	if (rp->width <= 0 || rp->height <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_rgb8: bad width/height");
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)rp->width * rp->height * 3;
	if (const int e = ensure_film(c, n); e != JP_OK) return e;
	float* const d_film = c->film.get<float>();
	if (const int e = ensure_rgb8(c, n); e != JP_OK) return e;
	unsigned char* stage = c->h_rgb8.reserve(n) == hipSuccess ? c->h_rgb8.get<unsigned char>() : rgb8_host;
	int st = render_impl(c, rp, d_film, false); if (st != JP_OK) return st;
	if (const int e = film_to_rgb8(c, d_film, rp->width, rp->height); e != JP_OK) return e;
	HIP_TRY(hipMemcpyAsync(stage, c->rgb8.get<void>(), n, hipMemcpyDeviceToHost, c->stream));
	if (film_host) HIP_TRY(hipMemcpyAsync(film_host, d_film, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (stage != rgb8_host) std::memcpy(rgb8_host, stage, n);
	return JP_OK;
}

int jp_synchronize(JpContext* c) { if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_synchronize: null context"); HIP_TRY(hipSetDevice(c->device)); HIP_TRY(hipStreamSynchronize(c->stream)); return JP_OK; }
int jp_set_profiling(JpContext* c, int enabled) { if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_profiling: null context"); c->profiling = enabled != 0; return JP_OK; }
int jp_get_counters(JpContext* c, JpCounters* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_counters: null argument");
	int st = finish_counters(c); if (st != JP_OK) return st;
	*out = c->counters; return JP_OK;
}
int jp_get_build_info(JpContext* c, JpBuildInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_build_info: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_get_build_info: no scene uploaded");
	out->built_on_device = c->build_on_device ? 1 : 0; out->traversal_mode = c->plan.trav_mode; out->bvh_nodes = c->bvh_nodes; out->bvh_height = c->bvh_height;
	out->device_build_ms = c->build_ms; out->libm_sincosf = c->sincosf_mode; out->lanes_last_render = c->last_lanes;
	out->fused_last_render = c->last_fused; out->fused_region = c->last_region; out->fused_workgroups = c->last_wgs;
	out->q4_nodes = c->plan.use_q4 ? c->plan.sv.n_q4 : 0; out->libm_xbsdf = c->libm_mode;
	out->certified_walk = (c->plan.cert && c->plan.persist != 0 && !c->cert_fell_back) ? 1 : 0;   // (what the refill kernels of the last render actually walked: the certified structures exist AND were used)
	out->certified_nodes = c->plan.cert ? c->plan.sv.n_q4 : 0; out->certified_eye_leaves = c->plan.cert ? c->cert_eye_leaves : 0;
	return JP_OK;
}

int jp_bsdf(JpContext* c, const JpBsdfDesc* d, int32_t n, const float* normal, const float* wo, const float* wi, const float* u,
            float* f_eval, float* pdf_eval, float* s_f, float* s_wi, float* s_pdf, int32_t* s_flags)
{
	if (!c || !d || n < 0 || !normal || !wo || !wi || !u || !f_eval || !pdf_eval || !s_f || !s_wi || !s_pdf || !s_flags) return fail(JP_ERR_INVALID_ARGUMENT, "jp_bsdf: null argument");
	if (d->kind < JP_BSDF_LAMBERT || d->kind > JP_BSDF_PHONG) return fail(JP_ERR_INVALID_ARGUMENT, "jp_bsdf: unknown BSDF kind");
	if ((d->kind == JP_BSDF_MICROFACET_REFLECTION || d->kind == JP_BSDF_MICROFACET_TRANSMISSION) && (d->distribution < JP_DIST_TROWBRIDGE_REITZ || d->distribution > JP_DIST_BECKMANN))
		return fail(JP_ERR_INVALID_ARGUMENT, "jp_bsdf: unknown microfacet distribution");
	if (d->kind == JP_BSDF_MICROFACET_REFLECTION && (d->fresnel < JP_FRESNEL_CONDUCTOR || d->fresnel > JP_FRESNEL_NOOP)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_bsdf: unknown Fresnel term");
	if (d->kind == JP_BSDF_FRESNEL_SPECULAR && d->eta_a != 1.0f) return fail(JP_ERR_UNSUPPORTED, "jp_bsdf: FFresnelSpecular is implemented for etaI = 1 (FGlassMaterial, material.h:72-75)");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	// scratch buffers kept in the context (a host FBSDF::Evalf is one event per call: no allocation per event); every copy checked
	const size_t cap = std::max<size_t>((size_t)n, 256);
	if (const int e = reserve_idle(c, c->bsdf_in, cap * 11 * 4); e != JP_OK) return e;
	if (const int e = reserve_idle(c, c->bsdf_out, cap * 11 * 4); e != JP_OK) return e;
	if (const int e = reserve_idle(c, c->bsdf_fl, cap * 4); e != JP_OK) return e;
	float *dn = c->bsdf_in.get<float>(), *dwo = dn + 3 * (size_t)n, *dwi = dn + 6 * (size_t)n, *du = dn + 9 * (size_t)n;
	float *df = c->bsdf_out.get<float>(), *dpe = df + 3 * (size_t)n, *dsf = df + 4 * (size_t)n, *dswi = df + 7 * (size_t)n, *dsp = df + 10 * (size_t)n;
	int* dfl = c->bsdf_fl.get<int>();
	HIP_TRY(hipMemcpyAsync(dn, normal, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(dwo, wo, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dwi, wi, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(du, u, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(k_bsdf, dim3(grid), dim3(JP_BLOCK), 0, c->stream, *d, n, (const float*)dn, (const float*)dwo, (const float*)dwi, (const float*)du, df, dpe, dsf, dswi, dsp, dfl);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(f_eval, df, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(pdf_eval, dpe, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(s_f, dsf, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(s_wi, dswi, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(s_pdf, dsp, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(s_flags, dfl, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_trace(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* hit, float* t, int32_t* prim, float* normal)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !hit || !t || !prim || !normal) return fail(JP_ERR_INVALID_ARGUMENT, "jp_trace: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_trace: no scene uploaded");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_o, b_d, b_t0, b_t1, b_t, b_n, b_hit, b_prim;           // per-call scratch: freed on every return
	float *d_o, *d_d, *d_t0, *d_t1, *d_t, *d_n; int *d_hit, *d_prim;
	HIP_TRY(reserve(b_o, d_o, (size_t)n * 12)); HIP_TRY(reserve(b_d, d_d, (size_t)n * 12)); HIP_TRY(reserve(b_t0, d_t0, (size_t)n * 4)); HIP_TRY(reserve(b_t1, d_t1, (size_t)n * 4));
	HIP_TRY(reserve(b_t, d_t, (size_t)n * 4)); HIP_TRY(reserve(b_n, d_n, (size_t)n * 12)); HIP_TRY(reserve(b_hit, d_hit, (size_t)n * 4)); HIP_TRY(reserve(b_prim, d_prim, (size_t)n * 4));
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	const TraceLaunch tk = trace_kernel(c->plan, c->opt.trace_walk, c->opt.reserved[0] == 1);
	hipLaunchKernelGGL(tk.trace, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, tk.depth, n, d_o, d_d, d_t0, d_t1, d_hit, d_t, d_prim, d_n);
	HIP_TRY(hipMemcpyAsync(hit, d_hit, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(t, d_t, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(prim, d_prim, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(normal, d_n, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_occluded(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* occluded, int32_t* walk_out)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !occluded) return fail(JP_ERR_INVALID_ARGUMENT, "jp_occluded: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_occluded: no scene uploaded");
	const OccludedLaunch ok = occluded_kernel(c->plan, c->opt.trace_walk, c->opt.reserved[0] == 1);
	if (walk_out) *walk_out = ok.walk;
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_o, b_d, b_t0, b_t1, b_occ;                             // per-call scratch: freed on every return
	float *d_o, *d_d, *d_t0, *d_t1; int* d_occ;
	HIP_TRY(reserve(b_o, d_o, (size_t)n * 12)); HIP_TRY(reserve(b_d, d_d, (size_t)n * 12)); HIP_TRY(reserve(b_t0, d_t0, (size_t)n * 4)); HIP_TRY(reserve(b_t1, d_t1, (size_t)n * 4));
	HIP_TRY(reserve(b_occ, d_occ, (size_t)n * 4));
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(ok.occluded, dim3(grid), dim3(JP_BLOCK), ok.lds, c->stream, c->plan.sv, ok.depth, n, d_o, d_d, d_t0, d_t1, d_occ);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(occluded, d_occ, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_get_texture_info(JpContext* c, JpTextureInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_info: set JpTextureInfo.struct_bytes to sizeof(JpTextureInfo)");
	JpTextureInfo i; std::memset(&i, 0, sizeof(i));
	i.n_textures = c->plan.textured ? c->n_textures : 0; i.n_textured_materials = c->n_tex_mats; i.texel_bytes_device = c->texel_bytes; i.textured_last_render = c->last_textured;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);                                                   // (a shorter struct of the caller is truncated)
	return JP_OK;
}

int jp_surface(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* prim, float* uv, float* albedo)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !prim || !uv || !albedo) return fail(JP_ERR_INVALID_ARGUMENT, "jp_surface: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_surface: no scene uploaded");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_in, b_uv, b_a, b_prim; float *d_in, *d_uv, *d_a; int* d_prim;   // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 32)); HIP_TRY(reserve(b_uv, d_uv, (size_t)n * 8)); HIP_TRY(reserve(b_a, d_a, (size_t)n * 12)); HIP_TRY(reserve(b_prim, d_prim, (size_t)n * 4));
	float *d_o = d_in, *d_d = d_in + 3 * (size_t)n, *d_t0 = d_in + 6 * (size_t)n, *d_t1 = d_in + 7 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	const TraceLaunch tk = trace_kernel(c->plan, 0);                // the walk jp_trace takes by default (what the render's closest-hit rays walk)
	if (c->plan.proc_on > 0)
	{   // a scene with a procedural record (jp_procedural.h): k_surface's twin reports the record's colour at width 0
		const SurfaceProcKernel sk = by_trace_mode(tk.mode & 15, [](auto m) -> SurfaceProcKernel { return k_surface_p<decltype(m)::value>; });
		if (!sk) return fail(JP_ERR_UNSUPPORTED, "jp_surface: no instance for this walk on a scene with procedural textures");
		hipLaunchKernelGGL(sk, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.tv, tk.depth, n, d_o, d_d, d_t0, d_t1, d_prim, d_uv, d_a, c->plan.sm, c->plan.proc);
	}
	else hipLaunchKernelGGL(tk.surface, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.tv, tk.depth, n, d_o, d_d, d_t0, d_t1, d_prim, d_uv, d_a, c->plan.sm);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(prim, d_prim, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(uv, d_uv, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(albedo, d_a, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

} // extern "C"

// Diagnostic, outside the ABI structs: which shadow kernel shadow_kernel picks for the uploaded scene under the options in force.
// 0: a lane-refill kernel, 1: k_shadow<mode> with every feature in it, 2: k_shadow<2, FeatFlat>, 3: k_shadow_pair
extern "C" int jp_dbg_shadow_kernel(JpContext* c, int* which_out)
{
	if (!c || !which_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_dbg_shadow_kernel: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_dbg_shadow_kernel: no scene uploaded");
	const ShadowLaunch sk = shadow_kernel(c->plan, c->q.R ? c->q.R : JP_BLOCK, c->opt.reserved[0] == 1);
	*which_out = sk.refill ? 0 : (sk.plain == (ShadowKernel)k_shadow_pair ? 3 : (sk.plain == (ShadowKernel)k_shadow<2, FeatFlat> ? 2 : 1));
	return JP_OK;
}

// The same for the closest-hit kernel extend_kernel picks.  0: a lane-refill kernel, 1: k_extend<mode> with every feature in it, 2: k_extend<2, FeatFlat>, 3: k_extend_pool
extern "C" int jp_dbg_extend_kernel(JpContext* c, int* which_out)
{
	if (!c || !which_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_dbg_extend_kernel: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_dbg_extend_kernel: no scene uploaded");
	const ExtendLaunch ek = extend_kernel(c->plan, c->opt.reserved[0] == 1);
	*which_out = ek.refill ? 0 : (ek.plain == (ExtendKernel)k_extend_pool ? 3 : (ek.plain == (ExtendKernel)k_extend<2, FeatFlat> ? 2 : 1));
	return JP_OK;
}

#if defined(JP_SHADE_TIMING) || defined(JP_TRAV_TIMING)
extern "C" int jp_dbg_shade_timing(unsigned long long* out16)
{
	unsigned long long z[16] = { 0 };
	if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_shade_t), sizeof(z)) != hipSuccess) return -1;
	if (hipMemcpyToSymbol(HIP_SYMBOL(g_shade_t), z, sizeof(z)) != hipSuccess) return -1;
	return 0;
}
#endif

#ifdef JP_WALK_STATS
extern "C" int jp_dbg_walk_stats(unsigned long long* out8)
{
	unsigned long long z[8] = { 0 };
	if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(jp::g_walk_stats), sizeof(z)) != hipSuccess) return -1;
	if (hipMemcpyToSymbol(HIP_SYMBOL(jp::g_walk_stats), z, sizeof(z)) != hipSuccess) return -1;
	return 0;
}
extern "C" int jp_dbg_turn_stats(unsigned long long* out32)
{
	unsigned long long z[32] = { 0 };
	if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(jp::g_turn_stats), sizeof(z)) != hipSuccess) return -1;
	if (hipMemcpyToSymbol(HIP_SYMBOL(jp::g_turn_stats), z, sizeof(z)) != hipSuccess) return -1;
	return 0;
}
#endif

#ifdef JP_PATH_TIMING
extern "C" int jp_dbg_path_timing(unsigned long long* out16)
{
	unsigned long long z[16] = { 0 };
	if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_path_t), sizeof(z)) != hipSuccess) return -1;
	if (hipMemcpyToSymbol(HIP_SYMBOL(g_path_t), z, sizeof(z)) != hipSuccess) return -1;
	return 0;
}
#endif

