// jet-pbrt_amd/csrc/jp_denoise.h -- guides and denoising (include/jetpbrt_amd.h "Guides and denoising", DESIGN.md "Denoiser"): the first-hit feature
// buffers of a frame (k_guides) and the edge-avoiding a-trous wavelet filter they steer (k_atrous_pack, k_atrous), with their entry points.
// Included by jp_kernels.hip LAST, after the kernels and the host runtime: nothing before it refers to anything in here, the new kernels are
// launched from the new entry points only, and every kernel above compiles to the instructions it compiled to without this file
// (tools/asm_kernel_diff.py).
#pragma once

// ---------------------------------------------------------------------------------------------------------------------
// k_guides: per pixel, guide_spp camera rays -- the ray k_raygen forms for sample s of the pixel -- through k_surface's walk; albedo, normal
// and depth of the closest hits summed in sample order by the one thread that owns the pixel, then scaled by 1.0f / guide_spp.
// ---------------------------------------------------------------------------------------------------------------------
struct GuideConst
{
	int width, height, spp;
	unsigned int seed;
	int sampler_debug;
	int band_rows, shard_index, shard_count;
};

// kSmooth (k_guides_smooth, scenes with vertex normals; jp_normals.h): the normal of a hit on a smooth triangle is the shading normal Ns the render uses there
// kLens (k_guides_lens, k_guides_smooth_lens; jp_set_lens in force): the lens ray of the sample, draws 2 and 3 of its key -- instances of their own, so the pinhole's
// kernels keep their registers and their instruction streams
// kMapped (k_guides_mapped, k_guides_mapped_lens, scenes with normal maps; jp_normal_map.h): the normal is the Ns the render uses there -- the smooth triangle's Ns where the scene has vertex
// normals (nv.prim_vn may be null), then the material's map on top; instances of their own again
// sm (jp_tex_sampling.h; both pointers null: no active record): the sampling records of the textures and the maps, a runtime branch in every form -- the albedo and the
// normal guide describe the surface the render shades
// mv (jp_mipmap.h; mv.tex null: no pyramid): the albedo follows the mip the render's camera ray reads at the first hit, one runtime branch again
// pv (jp_procedural.h; pv.tex null: no procedural record): likewise the procedural colour at the first hit's footprint
// pp (jp_projection.h; kind 0: the pinhole): the projected ray of the sample, one wave-uniform runtime branch in the kernels without a lens (k_guides, k_guides_smooth,
// k_guides_mapped; a lens together with a projection is refused, so the lens twins never see one).  The host puts the projection's cone spread into mv.gamma0
template <int kMode, bool kSmooth, bool kLens, bool kMapped = false>
__device__ __forceinline__ void guides_body(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, const NormView& nv, const JpLensPlan* lp, const SampView& sm, const MipView& mv, const ProcView& pv, const JpProjectionPlan* pp = nullptr, const NMapView* mp = nullptr)
{
	SceneAccess<kMode> acc(sc, depth);
	const int npix = gc.width * gc.height;
	const float inv = 1.0f / (float)gc.spp;
	for (int pix = blockIdx.x * JP_BLOCK + threadIdx.x; pix < npix; pix += gridDim.x * JP_BLOCK)
	{
		const int y = pix / gc.width, x = pix - y * gc.width;
		V3 A = splat(0), N = splat(0); float T = 0.f;
		if ((y / gc.band_rows) % gc.shard_count == gc.shard_index)
		{
			for (int s = 0; s < gc.spp; s++)
			{
				const uint32_t key = jp_rng_key(gc.seed, (uint32_t)x, (uint32_t)y, (uint32_t)s);
				const float fx = (float)x + (gc.sampler_debug ? 0.5f : jp_rng_float(key, 0)), fy = (float)y + (gc.sampler_debug ? 0.5f : jp_rng_float(key, 1));
				V3 ro, rd;                                                                          // k_raygen's ray
				if constexpr (kLens) camera_ray<true>(sc.cam, lp, fx, fy, gc.sampler_debug ? 0.5f : jp_rng_float(key, 2), gc.sampler_debug ? 0.5f : jp_rng_float(key, 3), ro, rd);
				else if (pp->kind != JP_PROJ_PERSPECTIVE) projected_ray(sc.cam, *pp, fx, fy, ro, rd);
				else camera_ray<false>(sc.cam, nullptr, fx, fy, 0.f, 0.f, ro, rd);
				float tmax = JP_INF;
				const int h = acc.template trace<false>(sc, ro, rd, 0.001f, tmax);
				V3 a = splat(1), n = splat(0); float t = 0.f;
				if (h >= 0)
				{
					const int4 meta = sc.meta[h];
					const float4 g3 = sc.prims[4 * h + 3]; const int type = __float_as_int(g3.w);
					const V3 p = ro + tmax * rd;
					if (type == JP_SHAPE_TRIANGLE) n = xyz(g3);                                       // k_trace's normal
					else if (type == JP_SHAPE_RECTANGLE) n = dot(xyz(g3), rd) <= 0 ? xyz(g3) : -xyz(g3);
					else if (type == JP_SHAPE_DISK) n = xyz(sc.prims[4 * h + 1]);
					else n = normalize(p - xyz(sc.prims[4 * h]));
					if constexpr (kMapped) n = mapped_shading_normal(sc.prims, nv, *mp, h, meta.x, meta.y, p, n, sm.map);
					else if (kSmooth) shading_normal(sc.prims, nv, h, meta.x, p, n);
					t = tmax;
					const int mat = meta.y;
					if (mat >= 0)
					{   // k_surface's colour; (1,1,1) stays where that is 0 by definition
						const int mtype = sc.mat_type[mat];
						const int tx = tv.mat_tex ? tv.mat_tex[mat] : -1;
						if (tx >= 0 && pv.tex) a = tex_color(tv, proc_sample(sc.prims, tv, sm, mv, pv, h, meta.x, tx, p, mv.gamma0 * tmax));   // a scene with a procedural record: its colour at the first hit's cone (and the mip's, where mv.tex)
						else if (tx >= 0 && mv.tex) { float rho; a = tex_color(tv, tex_sample_m(sc.prims, tv, sm, mv, h, meta.x, tx, p, mv.gamma0 * tmax, rho)); }   // the first hit's cone: width = gamma0 * t
						else if (tx >= 0) a = tex_color(tv, tex_sample_s(tv, sm.tex, tx, tex_uv(sc.prims, tv, h, meta.x, p), p));
						else if (mtype == JP_MAT_MATTE || mtype == JP_MAT_MIRROR || mtype == JP_MAT_PLASTIC) a = xyz(sc.mats[4 * mat]);
					}
				}
				A = A + a; N = N + n; T = T + t;
			}
			A = A * inv; N = N * inv; T = T * inv;
		}
		if (albedo) { albedo[3 * pix] = A.x; albedo[3 * pix + 1] = A.y; albedo[3 * pix + 2] = A.z; }
		if (normal) { normal[3 * pix] = N.x; normal[3 * pix + 1] = N.y; normal[3 * pix + 2] = N.z; }
		if (dist) dist[pix] = T;
	}
}
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, SampView sm, MipView mv, ProcView pv, JpProjectionPlan pp)
{
	guides_body<kMode, false, false>(sc, tv, depth, gc, albedo, normal, dist, NormView(), nullptr, sm, mv, pv, &pp);
}
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides_smooth(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, NormView nv, SampView sm, MipView mv, ProcView pv, JpProjectionPlan pp)
{
	guides_body<kMode, true, false>(sc, tv, depth, gc, albedo, normal, dist, nv, nullptr, sm, mv, pv, &pp);
}
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides_lens(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, JpLensPlan lp, SampView sm, MipView mv, ProcView pv)
{
	guides_body<kMode, false, true>(sc, tv, depth, gc, albedo, normal, dist, NormView(), &lp, sm, mv, pv);
}
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides_smooth_lens(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, NormView nv, JpLensPlan lp, SampView sm, MipView mv, ProcView pv)
{
	guides_body<kMode, true, true>(sc, tv, depth, gc, albedo, normal, dist, nv, &lp, sm, mv, pv);
}

template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides_mapped(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, NormView nv, NMapView mp, SampView sm, MipView mv, ProcView pv, JpProjectionPlan pp)
{
	guides_body<kMode, false, false, true>(sc, tv, depth, gc, albedo, normal, dist, nv, nullptr, sm, mv, pv, &pp, &mp);
}
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_guides_mapped_lens(SceneView sc, TexView tv, int depth, GuideConst gc, float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ dist, NormView nv, NMapView mp, JpLensPlan lp, SampView sm, MipView mv, ProcView pv)
{
	guides_body<kMode, false, true, true>(sc, tv, depth, gc, albedo, normal, dist, nv, &lp, sm, mv, pv, nullptr, &mp);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_atrous: one iteration of the filter.  Per pixel two 16-byte records: (c.rgb, z) -- ping-pong, the colour changes every iteration -- and
// (n.xyz, -), so a tap is two dwordx4 loads; guides stay fp32 (the definition is exact).  A workgroup is a 32 x 8 pixel tile: a wave reads two
// 512-byte row segments per tap row, and the 25 taps of neighbouring pixels meet in L1 / L2 (steps 1, 2) or L2 / MALL (steps >= 4).
// k_atrous_pack builds the records once (demodulation: three divisions per pixel instead of three per tap); the last iteration re-modulates,
// clamps and writes the film layout.
// ---------------------------------------------------------------------------------------------------------------------
struct AtrousConst
{
	int width, height, step;
	float kc, kn, kz;
};
#define JP_ATROUS_TW 32
#define JP_ATROUS_TH (JP_BLOCK / JP_ATROUS_TW)

__global__ void __launch_bounds__(JP_BLOCK) k_atrous_pack(int npix, const float* __restrict__ film, const float* __restrict__ albedo, const float* __restrict__ normal,
                                                           const float* __restrict__ dist, float4* __restrict__ cz, float4* __restrict__ nr)
{
	for (int p = blockIdx.x * JP_BLOCK + threadIdx.x; p < npix; p += gridDim.x * JP_BLOCK)
	{
		float ar = 1.f, ag = 1.f, ab = 1.f;
		if (albedo) { ar = smax(albedo[3 * p], 0.001f); ag = smax(albedo[3 * p + 1], 0.001f); ab = smax(albedo[3 * p + 2], 0.001f); }
		cz[p] = make_float4(film[3 * p] / ar, film[3 * p + 1] / ag, film[3 * p + 2] / ab, dist[p]);
		nr[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], 0.f);
	}
}

template <bool kLast>
__global__ void __launch_bounds__(JP_BLOCK) k_atrous(AtrousConst ac, const float4* __restrict__ cz, const float4* __restrict__ nr, float4* __restrict__ cz_out,
                                                      const float* __restrict__ albedo, float* __restrict__ out)
{
	const int x = blockIdx.x * JP_ATROUS_TW + (threadIdx.x & (JP_ATROUS_TW - 1)), y = blockIdx.y * JP_ATROUS_TH + (threadIdx.x / JP_ATROUS_TW);
	if (x >= ac.width || y >= ac.height) return;
	const int p = y * ac.width + x;
	const float4 cp = cz[p], np = nr[p];
	float nr_ = 0.f, ng_ = 0.f, nb_ = 0.f, den = 0.f;
	#pragma unroll
	for (int dy = -2; dy <= 2; dy++)
	{
		const int qy = y + dy * ac.step;
		if (qy < 0 || qy >= ac.height) continue;
		const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
		#pragma unroll
		for (int dx = -2; dx <= 2; dx++)
		{
			const int qx = x + dx * ac.step;
			if (qx < 0 || qx >= ac.width) continue;
			const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
			const float hh = hy * hx;
			const int q = qy * ac.width + qx;
			const float4 cq = cz[q], nq = nr[q];
			const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
			const float dc = (dr * dr + dg * dg) + db * db;
			const float ex = np.x - nq.x, ey = np.y - nq.y, ez = np.z - nq.z;
			const float dn = (ex * ex + ey * ey) + ez * ez;
			const float m = smax(smax(cp.w, cq.w), 1e-20f);
			const float rz = (cp.w - cq.w) / m;
			const float dz = rz * rz;
			const float w = hh / (((1.f + dc * ac.kc) * (1.f + dn * ac.kn)) * (1.f + dz * ac.kz));
			nr_ += w * cq.x; ng_ += w * cq.y; nb_ += w * cq.z; den += w;
		}
	}
	const float r = nr_ / den, g = ng_ / den, b = nb_ / den;             // (the centre tap is always there: den >= 9/64)
	if (!kLast) cz_out[p] = make_float4(r, g, b, cp.w);
	else
	{
		float ar = 1.f, ag = 1.f, ab = 1.f;
		if (albedo) { ar = smax(albedo[3 * p], 0.001f); ag = smax(albedo[3 * p + 1], 0.001f); ab = smax(albedo[3 * p + 2], 0.001f); }
		out[3 * p] = clampf(r * ar, 0.f, 1.f); out[3 * p + 1] = clampf(g * ag, 0.f, 1.f); out[3 * p + 2] = clampf(b * ab, 0.f, 1.f);
	}
}

// k_atrous_unpack_hdr: the last step while the context's film state has hdr = 1 (jp_set_film): the last iteration then runs as k_atrous<false>, and this
// kernel re-modulates its records with the a of k_atrous_pack and writes max(c_n * a, 0) in the film layout -- the values k_atrous<true> clamps to 1, one
// pass of 28 bytes per pixel more, and the two instances of k_atrous stay the kernels they were
__global__ void __launch_bounds__(JP_BLOCK) k_atrous_unpack_hdr(int npix, const float4* __restrict__ cz, const float* __restrict__ albedo, float* __restrict__ out)
{
	for (int p = blockIdx.x * JP_BLOCK + threadIdx.x; p < npix; p += gridDim.x * JP_BLOCK)
	{
		float ar = 1.f, ag = 1.f, ab = 1.f;
		if (albedo) { ar = smax(albedo[3 * p], 0.001f); ag = smax(albedo[3 * p + 1], 0.001f); ab = smax(albedo[3 * p + 2], 0.001f); }
		const float4 c = cz[p];
		out[3 * p] = smax(c.x * ar, 0.f); out[3 * p + 1] = smax(c.y * ag, 0.f); out[3 * p + 2] = smax(c.z * ab, 0.f);
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace
{
#define JP_DENOISE_SIGMA_COLOR  1.0f
#define JP_DENOISE_SIGMA_NORMAL 0.1f
#define JP_DENOISE_SIGMA_DEPTH  0.03f

typedef void (*GuideKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, SampView, MipView, ProcView, JpProjectionPlan);
typedef void (*GuideSmoothKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, NormView, SampView, MipView, ProcView, JpProjectionPlan);
typedef void (*GuideLensKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, JpLensPlan, SampView, MipView, ProcView);
typedef void (*GuideSmoothLensKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, NormView, JpLensPlan, SampView, MipView, ProcView);
typedef void (*GuideMappedKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, NormView, NMapView, SampView, MipView, ProcView, JpProjectionPlan);
typedef void (*GuideMappedLensKernel)(SceneView, TexView, int, GuideConst, float*, float*, float*, NormView, NMapView, JpLensPlan, SampView, MipView, ProcView);
struct GuideLaunch { GuideKernel k; size_t lds; int depth; GuideSmoothKernel smooth; GuideLensKernel lens; GuideSmoothLensKernel smooth_lens; GuideMappedKernel mapped; GuideMappedLensKernel mapped_lens; };   // smooth: the twin a scene with vertex normals runs; lens: the twins of jp_set_lens
template <int M> GuideLaunch guide_row(size_t lds, int depth) { GuideLaunch g = { k_guides<M>, lds, depth, k_guides_smooth<M>, k_guides_lens<M>, k_guides_smooth_lens<M>, k_guides_mapped<M>, k_guides_mapped_lens<M> }; return g; }
// the walk trace_kernel(p, 0) gives jp_surface
GuideLaunch guide_kernel(const ScenePlan& p)
{
	const size_t q4lds = (size_t)p.stack_depth_q4 * JP_BLOCK * sizeof(int);
	if (p.trav_mode == 5 && p.cert && q4lds <= 64 * 1024) return guide_row<6>(q4lds, p.stack_depth_q4);
	if (p.trav_mode == 5) return guide_row<5>(p.lds_bytes, p.stack_depth);
	if (p.use_q4 && q4lds <= 64 * 1024) return guide_row<4>(q4lds, p.stack_depth_q4);
	return p.trav_mode == 2 ? guide_row<2>(p.lds_bytes, p.stack_depth) : (p.trav_mode == 1 ? guide_row<1>(p.lds_bytes, p.stack_depth) : guide_row<0>(p.lds_bytes, p.stack_depth));
}

int ensure_events(JpContext* c)
{
	for (hipEvent_t* e : { &c->dn_ev[0], &c->dn_ev[1], &c->gd_ev[0], &c->gd_ev[1] }) if (!*e) HIP_TRY(hipEventCreate(e));
	return JP_OK;
}

int guides_check(JpContext* c, const JpRenderParams* rp, int32_t guide_spp, GuideConst& gc)
{
	if (!c || !rp) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_guides: null argument");
	if (rp->width <= 0 || rp->height <= 0 || (long long)rp->width * rp->height > (1ll << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_guides: bad width/height");
	if (guide_spp < 1 || guide_spp > 1024) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_guides: guide_spp must be 1 .. 1024");
	if (rp->sampler_mode != JP_SAMPLER_COUNTER && rp->sampler_mode != JP_SAMPLER_DEBUG) return fail(JP_ERR_UNSUPPORTED, "jp_render_guides: the device path implements the counter sampler only (the sequential mt19937_64 stream is not reproducible in parallel)");
	gc.width = rp->width; gc.height = rp->height; gc.spp = guide_spp; gc.seed = rp->seed; gc.sampler_debug = rp->sampler_mode == JP_SAMPLER_DEBUG ? 1 : 0;
	gc.band_rows = rp->band_rows > 0 ? rp->band_rows : 20;
	gc.shard_count = rp->shard_count > 1 ? rp->shard_count : 1;
	gc.shard_index = gc.shard_count > 1 ? rp->shard_index : 0;
	if (gc.shard_index < 0 || gc.shard_index >= gc.shard_count) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_guides: shard_index out of range");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_render_guides: no scene uploaded");
	return JP_OK;
}

int guides_launch(JpContext* c, const GuideConst& gc, float* albedo, float* normal, float* dist)
{
	if (const int e = ensure_events(c); e != JP_OK) return e;
	const GuideLaunch gk = guide_kernel(c->plan);
	const int npix = gc.width * gc.height;
	const int grid = std::min(c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK);
	JpLensPlan lp;
	if (const int e = lens_plan_of(c, lp); e != JP_OK) return e;
	JpProjectionPlan pp;                                                 // jp_set_projection: sample s stays the camera ray of sample s of the render, with its cone spread
	if (const int e = proj_plan_of(c, pp); e != JP_OK) return e;
	MipView mv = c->plan.mv;
	if (c->proj_on) mv.gamma0 = pp.gamma0;
	HIP_TRY(hipEventRecord(c->gd_ev[0], c->stream));
	if (c->lens_on)
	{   // jp_set_lens: sample s stays the camera ray of sample s of the render
		if (c->plan.mapped) hipLaunchKernelGGL(gk.mapped_lens, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, c->plan.nv, c->plan.mp, lp, c->plan.sm, c->plan.mv, c->plan.proc);
		else if (c->plan.smooth) hipLaunchKernelGGL(gk.smooth_lens, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, c->plan.nv, lp, c->plan.sm, c->plan.mv, c->plan.proc);
		else hipLaunchKernelGGL(gk.lens, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, lp, c->plan.sm, c->plan.mv, c->plan.proc);
	}
	else if (c->plan.mapped) hipLaunchKernelGGL(gk.mapped, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, c->plan.nv, c->plan.mp, c->plan.sm, mv, c->plan.proc, pp);
	else if (c->plan.smooth) hipLaunchKernelGGL(gk.smooth, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, c->plan.nv, c->plan.sm, mv, c->plan.proc, pp);
	else hipLaunchKernelGGL(gk.k, dim3(grid), dim3(JP_BLOCK), gk.lds, c->stream, c->plan.sv, c->plan.tv, gk.depth, gc, albedo, normal, dist, c->plan.sm, mv, c->plan.proc, pp);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->gd_ev[1], c->stream));
	c->gd_timed = true; c->last_guide_spp = gc.spp;
	return JP_OK;
}

struct DenoiseSetup { int width, height, iterations; float sc, sn, sz; bool demod; };
int denoise_check(JpContext* c, const JpDenoiseParams* dp, const void* film, const void* albedo, const void* normal, const void* dist, const void* out, DenoiseSetup& s)
{
	if (!c || !dp) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: null argument");
	if (dp->struct_bytes < (int32_t)sizeof(JpDenoiseParams)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: set JpDenoiseParams.struct_bytes to sizeof(JpDenoiseParams)");
	if (dp->width <= 0 || dp->height <= 0 || (long long)dp->width * dp->height > (1ll << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: bad width/height");
	if (dp->iterations < 0 || dp->iterations > 6) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: iterations must be 1 .. 6 (0: the default, 5)");
	for (const float v : { dp->sigma_color, dp->sigma_normal, dp->sigma_depth })
		if (!(v >= 0.f) || !std::isfinite(v)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: a sigma must be positive and finite (0: the default)");
	if (dp->demodulate < -1 || dp->demodulate > 1) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: demodulate must be 0, 1 or -1");
	s.demod = dp->demodulate >= 0;
	if (!film || !normal || !dist || !out || (s.demod && !albedo)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: null buffer");
	s.width = dp->width; s.height = dp->height; s.iterations = dp->iterations ? dp->iterations : 5;
	s.sc = dp->sigma_color != 0.f ? dp->sigma_color : JP_DENOISE_SIGMA_COLOR; s.sn = dp->sigma_normal != 0.f ? dp->sigma_normal : JP_DENOISE_SIGMA_NORMAL;
	s.sz = dp->sigma_depth != 0.f ? dp->sigma_depth : JP_DENOISE_SIGMA_DEPTH;
	// out may not overlap an input
	const size_t n = (size_t)s.width * s.height * sizeof(float);
	const char* o0 = (const char*)out; const char* o1 = o0 + 3 * n;
	const struct { const void* p; size_t bytes; } in[4] = { { film, 3 * n }, { albedo, 3 * n }, { normal, 3 * n }, { dist, n } };
	for (const auto& i : in) if (i.p && (const char*)i.p < o1 && o0 < (const char*)i.p + i.bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise: out overlaps an input");
	return JP_OK;
}

int denoise_launch(JpContext* c, const DenoiseSetup& s, const float* film, const float* albedo, const float* normal, const float* dist, float* out)
{
	HIP_TRY(hipSetDevice(c->device));
	if (const int e = ensure_events(c); e != JP_OK) return e;
	const size_t npix = (size_t)s.width * s.height;
	for (DevBuf* b : { &c->dn_cz[0], &c->dn_cz[1], &c->dn_nr })      // the records: two colour buffers and the normals, 48 bytes per pixel
		if (const int e = reserve_idle(c, *b, npix * 16); e != JP_OK) return e;
	float4* const cz[2] = { c->dn_cz[0].get<float4>(), c->dn_cz[1].get<float4>() }; float4* const nr = c->dn_nr.get<float4>();
	const float kn = 1.0f / (s.sn * s.sn), kz = 1.0f / (s.sz * s.sz), sc2 = s.sc * s.sc;
	const float* alb = s.demod ? albedo : nullptr;
	HIP_TRY(hipEventRecord(c->dn_ev[0], c->stream));
	hipLaunchKernelGGL(k_atrous_pack, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream,
	                   (int)npix, film, alb, normal, dist, cz[0], nr);
	const dim3 grid((s.width + JP_ATROUS_TW - 1) / JP_ATROUS_TW, (s.height + JP_ATROUS_TH - 1) / JP_ATROUS_TH);
	float pow4 = 1.0f;
	for (int i = 0; i < s.iterations; i++, pow4 *= 4.0f)
	{
		const AtrousConst ac = { s.width, s.height, 1 << i, pow4 / sc2, kn, kz };
		const float4* src = cz[i & 1]; float4* dst = cz[(i & 1) ^ 1];
		const bool hdr = c->film_on && c->film_state.hdr;           // jp_set_film: the unclamped last step (k_atrous_unpack_hdr)
		if (i + 1 < s.iterations || hdr) hipLaunchKernelGGL(k_atrous<false>, grid, dim3(JP_BLOCK), 0, c->stream, ac, src, (const float4*)nr, dst, (const float*)nullptr, (float*)nullptr);
		if (i + 1 < s.iterations) continue;
		if (hdr) hipLaunchKernelGGL(k_atrous_unpack_hdr, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream, (int)npix, (const float4*)dst, alb, out);
		else hipLaunchKernelGGL(k_atrous<true>, grid, dim3(JP_BLOCK), 0, c->stream, ac, src, (const float4*)nr, (float4*)nullptr, alb, out);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->dn_ev[1], c->stream));
	c->dn_timed = true; c->last_dn = s.iterations; c->last_dn_sigma[0] = s.sc; c->last_dn_sigma[1] = s.sn; c->last_dn_sigma[2] = s.sz; c->last_dn_demod = s.demod ? 1 : 0;
	return JP_OK;
}

// staging area of the host variants (floats)
int ensure_stage(JpContext* c, size_t n) { return reserve_idle(c, c->dn_stage, n * sizeof(float)); }
}

extern "C" {

int jp_render_guides_device(JpContext* c, const JpRenderParams* rp, int32_t guide_spp, void* albedo_dev, void* normal_dev, void* depth_dev, int sync)
{
	GuideConst gc;
	if (const int e = guides_check(c, rp, guide_spp, gc); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	if (const int e = guides_launch(c, gc, (float*)albedo_dev, (float*)normal_dev, (float*)depth_dev); e != JP_OK) return e;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_render_guides(JpContext* c, const JpRenderParams* rp, int32_t guide_spp, float* albedo, float* normal, float* depth)
{
	GuideConst gc;
	if (const int e = guides_check(c, rp, guide_spp, gc); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)gc.width * gc.height;
	if (const int e = ensure_stage(c, 7 * n); e != JP_OK) return e;
	float *da = c->dn_stage.get<float>(), *dn = da + 3 * n, *dz = da + 6 * n;
	if (const int e = guides_launch(c, gc, albedo ? da : nullptr, normal ? dn : nullptr, depth ? dz : nullptr); e != JP_OK) return e;
	if (albedo) HIP_TRY(hipMemcpyAsync(albedo, da, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (normal) HIP_TRY(hipMemcpyAsync(normal, dn, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (depth) HIP_TRY(hipMemcpyAsync(depth, dz, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_denoise_device(JpContext* c, const JpDenoiseParams* dp, const void* film_dev, const void* albedo_dev, const void* normal_dev, const void* depth_dev, void* out_dev, int sync)
{
	DenoiseSetup s;
	if (const int e = denoise_check(c, dp, film_dev, albedo_dev, normal_dev, depth_dev, out_dev, s); e != JP_OK) return e;
	if (const int e = denoise_launch(c, s, (const float*)film_dev, (const float*)albedo_dev, (const float*)normal_dev, (const float*)depth_dev, (float*)out_dev); e != JP_OK) return e;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_denoise(JpContext* c, const JpDenoiseParams* dp, const float* film, const float* albedo, const float* normal, const float* depth, float* out)
{
	DenoiseSetup s;
	if (const int e = denoise_check(c, dp, film, albedo, normal, depth, out, s); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)s.width * s.height;
	if (const int e = ensure_stage(c, 13 * n); e != JP_OK) return e;
	float *df = c->dn_stage.get<float>(), *da = df + 3 * n, *dn = df + 6 * n, *dz = df + 9 * n, *dout = df + 10 * n;
	HIP_TRY(hipMemcpyAsync(df, film, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (s.demod) HIP_TRY(hipMemcpyAsync(da, albedo, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dn, normal, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dz, depth, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (const int e = denoise_launch(c, s, df, da, dn, dz, dout); e != JP_OK) return e;
	HIP_TRY(hipMemcpyAsync(out, dout, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

// jp_render, jp_render_guides, jp_denoise and the tone map of jp_render_rgb8 in one call: the film stays on the device between the stages
int jp_render_denoised(JpContext* c, const JpRenderParams* rp, int32_t guide_spp, const JpDenoiseParams* dp, float* film_host, uint8_t* rgb8_host, float* albedo, float* normal, float* depth)
{
	if (!c || !rp || (!film_host && !rgb8_host)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_denoised: null argument");
	GuideConst gc;
	if (const int e = guides_check(c, rp, guide_spp, gc); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)gc.width * gc.height;
	if (const int e = ensure_stage(c, 10 * n); e != JP_OK) return e;
	float *da = c->dn_stage.get<float>(), *dn = da + 3 * n, *dz = da + 6 * n, *dout = da + 7 * n;
	if (const int e = ensure_film(c, 3 * n); e != JP_OK) return e;
	float* const film = c->film.get<float>();
	DenoiseSetup s;
	if (dp)
	{
		JpDenoiseParams d = *dp; d.width = gc.width; d.height = gc.height;
		if (const int e = denoise_check(c, &d, film, da, dn, dz, dout, s); e != JP_OK) return e;
	}
	if (const int e = render_impl(c, rp, film, false); e != JP_OK) return e;
	if (const int e = guides_launch(c, gc, da, dn, dz); e != JP_OK) return e;
	const float* result = film;
	if (dp) { if (const int e = denoise_launch(c, s, film, da, dn, dz, dout); e != JP_OK) return e; result = dout; }
	if (rgb8_host)
	{
		if (const int e = ensure_rgb8(c, 3 * n); e != JP_OK) return e;
		if (const int e = film_to_rgb8(c, result, gc.width, gc.height); e != JP_OK) return e;
		HIP_TRY(hipMemcpyAsync(rgb8_host, c->rgb8.get<void>(), 3 * n, hipMemcpyDeviceToHost, c->stream));
	}
	if (film_host) HIP_TRY(hipMemcpyAsync(film_host, result, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (albedo) HIP_TRY(hipMemcpyAsync(albedo, da, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (normal) HIP_TRY(hipMemcpyAsync(normal, dn, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (depth) HIP_TRY(hipMemcpyAsync(depth, dz, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_get_denoise_info(JpContext* c, JpDenoiseInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_denoise_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_denoise_info: set JpDenoiseInfo.struct_bytes to sizeof(JpDenoiseInfo)");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	JpDenoiseInfo i; std::memset(&i, 0, sizeof(i));
	i.iterations = c->last_dn; i.sigma_color = c->last_dn_sigma[0]; i.sigma_normal = c->last_dn_sigma[1]; i.sigma_depth = c->last_dn_sigma[2];
	i.demodulated = c->last_dn_demod; i.guide_spp = c->last_guide_spp;
	float ms = 0.f;
	if (c->dn_timed && hipEventElapsedTime(&ms, c->dn_ev[0], c->dn_ev[1]) == hipSuccess) i.denoise_ms = ms;
	if (c->gd_timed && hipEventElapsedTime(&ms, c->gd_ev[0], c->gd_ev[1]) == hipSuccess) i.guides_ms = ms;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

} // extern "C"
