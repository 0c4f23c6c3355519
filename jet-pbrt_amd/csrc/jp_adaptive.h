// jet-pbrt_amd/csrc/jp_adaptive.h -- adaptive sampling: a render that stops each pixel by the variance of its own mean (include/jetpbrt_amd.h "Adaptive sampling",
// DESIGN.md "Adaptive sampling").  The rule is include/jp_adaptive.h, shared with the host.  Two parts, like jp_variance.h: part 1 (after jp_variance.h's in
// jp_kernels.hip: k_raygen_list and k_resolve_list, the twins of k_raygen and the resolve kernels that go through a pixel list; k_adapt_select, k_adapt_scan and
// k_adapt_compact, the test and the ordered compaction of the survivors; k_adapt_finish) and, with JP_ADAPTIVE_RUNTIME defined, part 2 LAST: the driver loop and the
// entry points.  Nothing runs unless one of the new entry points is called, and no kernel above changes: k_extend*, k_shade*, k_shadow* and the side kernels see
// slots and the key in beta.w only, so the bounces between the two twins are the launches of render_one.
#ifndef JP_ADAPTIVE_DEVICE_PART
#define JP_ADAPTIVE_DEVICE_PART
#include "../../include/jp_adaptive.h"

// ---------------------------------------------------------------------------------------------------------------------
// k_raygen_list: k_raygen through a list.  Slot = sample * n_act + position, position -> pix = list[position] (list null: the identity, the first pass); then
// k_raygen's pixel_of, key, camera_ray and records, into the same region layout with the same blk_q[0][b].  The chunks b, b + G, ... of a region, tail chunk
// included: n_act is any number (k_raygen's compact order needs npix / JP_BLOCK and is not offered here).
// ---------------------------------------------------------------------------------------------------------------------
template <bool kLens>
__global__ void __launch_bounds__(JP_BLOCK) k_raygen_list(SceneView sc, Queues q, RenderConst rc, DevCounters* cnt, typename LensArg<kLens>::type lp, const unsigned int* __restrict__ list, unsigned int n_act)
{
	const unsigned int total = n_act * (unsigned int)rc.sbatch;
	const unsigned int nchunks = (total + JP_BLOCK - 1) / JP_BLOCK;
	const unsigned int G = gridDim.x, b = blockIdx.x;
	if (b == 0 && threadIdx.x == 0) { cnt->n_queue[0] = total; cnt->n_queue[1] = 0; cnt->n_shadow = 0; }
	unsigned int filled = 0;
	const unsigned int K = (nchunks + G - 1) / G;
	for (unsigned int k = 0, j0 = 0; k < K; k++, j0 += JP_BLOCK)
	{
		const unsigned int c = b + k * G;
		if (c >= nchunks) break;
		const unsigned int slot = c * JP_BLOCK + threadIdx.x;
		if (slot < total)
		{
			const unsigned int i = b * q.R + j0 + threadIdx.x;
			const unsigned int sl = slot / n_act, pos = slot - sl * n_act;
			const int pix = list ? (int)list[pos] : (int)pos, s = rc.s0 + (int)sl;
			int x, y; pixel_of(rc, pix, x, y);
			const uint32_t key = jp_rng_key(rc.seed, (uint32_t)x, (uint32_t)y, (uint32_t)s);
			const float fx = (float)x + rngf(rc, key, 0), fy = (float)y + rngf(rc, key, 1);
			V3 o, dir;
			if constexpr (kLens) camera_ray<true>(sc.cam, &lp, fx, fy, rngf(rc, key, 2), rngf(rc, key, 3), o, dir);
			else camera_ray<false>(sc.cam, nullptr, fx, fy, 0.f, 0.f, o, dir);
			q.ray_o[0][i] = make_float4(o.x, o.y, o.z, __int_as_float((int)slot));
			q.ray_d[0][i] = make_float4(dir.x, dir.y, dir.z, __int_as_float(MK_FLAGS(0, 0, kLens ? 4 : 2)));
			q.beta[0][i] = make_float4(1.f, 1.f, 1.f, __int_as_float((int)key));
			q.lacc[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
		}
		const unsigned int left = total - c * JP_BLOCK;
		filled += left < JP_BLOCK ? left : JP_BLOCK;
	}
	if (threadIdx.x == 0) q.blk_q[0][b] = filled;
}

// k_raygen_list_proj: the same twin for k_raygen_proj (jp_set_projection in force)
__global__ void __launch_bounds__(JP_BLOCK) k_raygen_list_proj(SceneView sc, Queues q, RenderConst rc, DevCounters* cnt, JpProjectionPlan pp, const unsigned int* __restrict__ list, unsigned int n_act)
{
	const unsigned int total = n_act * (unsigned int)rc.sbatch;
	const unsigned int nchunks = (total + JP_BLOCK - 1) / JP_BLOCK;
	const unsigned int G = gridDim.x, b = blockIdx.x;
	if (b == 0 && threadIdx.x == 0) { cnt->n_queue[0] = total; cnt->n_queue[1] = 0; cnt->n_shadow = 0; }
	unsigned int filled = 0;
	const unsigned int K = (nchunks + G - 1) / G;
	for (unsigned int k = 0, j0 = 0; k < K; k++, j0 += JP_BLOCK)
	{
		const unsigned int c = b + k * G;
		if (c >= nchunks) break;
		const unsigned int slot = c * JP_BLOCK + threadIdx.x;
		if (slot < total)
		{
			const unsigned int i = b * q.R + j0 + threadIdx.x;
			const unsigned int sl = slot / n_act, pos = slot - sl * n_act;
			const int pix = list ? (int)list[pos] : (int)pos, s = rc.s0 + (int)sl;
			int x, y; pixel_of(rc, pix, x, y);
			const uint32_t key = jp_rng_key(rc.seed, (uint32_t)x, (uint32_t)y, (uint32_t)s);
			const float fx = (float)x + rngf(rc, key, 0), fy = (float)y + rngf(rc, key, 1);
			V3 o, dir;
			projected_ray(sc.cam, pp, fx, fy, o, dir);
			q.ray_o[0][i] = make_float4(o.x, o.y, o.z, __int_as_float((int)slot));
			q.ray_d[0][i] = make_float4(dir.x, dir.y, dir.z, __int_as_float(MK_FLAGS(0, 0, 2)));
			q.beta[0][i] = make_float4(1.f, 1.f, 1.f, __int_as_float((int)key));
			q.lacc[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
		}
		const unsigned int left = total - c * JP_BLOCK;
		filled += left < JP_BLOCK ? left : JP_BLOCK;
	}
	if (threadIdx.x == 0) q.blk_q[0][b] = filled;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_resolve_list: the resolve twin.  For list position pos (pixel list[pos]; list null: the identity) the batch's sbatch samples from sample index s0 enter the
// pixel's state in sample order: sum.xyz the unscaled rgb sum after the sample clamp, sum.w the count (int bits), mom = (mean, m2).  The state is zero before
// the first pass and stays in memory between the passes.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JP_BLOCK) k_resolve_list(const float4* __restrict__ lacc, unsigned int n_act, const unsigned int* __restrict__ list, int s0, int sbatch, float4* sum, float2* mom, float sample_clamp)
{
	for (unsigned int pos = blockIdx.x * JP_BLOCK + threadIdx.x; pos < n_act; pos += gridDim.x * JP_BLOCK)
	{
		const unsigned int pix = list ? list[pos] : pos;
		float4 a = sum[pix]; float2 m = mom[pix];
		for (int s = 0; s < sbatch; s++)
		{
			float4 l = lacc[(size_t)s * n_act + pos];
			if (sample_clamp > 0.f) jp_film_clamp_sample(sample_clamp, &l.x, &l.y, &l.z);
			a.x = a.x + l.x; a.y = a.y + l.y; a.z = a.z + l.z;
			jp_var_step(&m.x, &m.y, jp_var_luminance(l.x, l.y, l.z), s0 + s + 1);
		}
		a.w = __int_as_float(__float_as_int(a.w) + sbatch);
		sum[pix] = a; mom[pix] = m;
	}
}

// jp_adaptive_probe: caller-supplied samples [max_spp][npix][3] take the place of the paths' radiances, in the layout k_resolve_list reads
__global__ void __launch_bounds__(JP_BLOCK) k_adapt_probe_fill(float4* __restrict__ lacc, const float* __restrict__ samples, unsigned int npix, unsigned int n_act, const unsigned int* __restrict__ list, int s0, int sbatch)
{
	const size_t total = (size_t)n_act * sbatch;
	for (size_t slot = (size_t)blockIdx.x * JP_BLOCK + threadIdx.x; slot < total; slot += (size_t)gridDim.x * JP_BLOCK)
	{
		const unsigned int sl = (unsigned int)(slot / n_act), pos = (unsigned int)(slot - (size_t)sl * n_act);
		const unsigned int pix = list ? list[pos] : pos;
		const float* l = samples + 3 * ((size_t)(s0 + sl) * npix + pix);
		lacc[slot] = make_float4(l[0], l[1], l[2], 0.f);
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// The selection, three launches on one stream.  Workgroup b owns the shard-local pixels [256 b, 256 b + 256), wave w of it 64 consecutive ones; the active set is
// one 64-bit mask per wave (act[4 b + w], bit = lane), so positions never come from an atomic: the order of the next list is ascending pixel order by construction.
//   k_adapt_select   per pixel: jp_adapt_keep (the pass test of the pixel, or of its 3 x 3 neighbourhood) for the active ones; the wave's ballot is its new mask,
//                    the popcounts of the workgroup's four masks add up in LDS to blk_tot[b]
//   k_adapt_scan     one workgroup: the exclusive scan of blk_tot (each thread a contiguous run, the 256 run totals scanned in LDS) into blk_off; the total goes
//                    to the pinned word the host reads to size the next pass
//   k_adapt_compact  per wave: rank = mbcnt of its mask below the lane, base = blk_off[b] + the masks' popcounts of the waves before it (LDS); survivors write
//                    their pixel index to list[base + rank]
// ---------------------------------------------------------------------------------------------------------------------
struct AdaptConst
{
	JpAdaptShard sh;
	int npix;
	float threshold, floor;
	int dilate;
};

__global__ void __launch_bounds__(JP_BLOCK) k_adapt_select(AdaptConst ac, const float4* __restrict__ sum, const float2* __restrict__ mom, const unsigned long long* __restrict__ act_in,
                                                            unsigned long long* __restrict__ act_out, unsigned int* __restrict__ blk_tot)
{
	__shared__ unsigned int s_cnt[JP_BLOCK / 64];
	const int p = (int)(blockIdx.x * JP_BLOCK + threadIdx.x);
	const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	bool keep = false;
	if (p < ac.npix && ((act_in[blockIdx.x * (JP_BLOCK / 64) + wave] >> lane) & 1ull))
		keep = jp_adapt_keep(&ac.sh, p, (const float*)mom, (const int32_t*)sum + 3, 4, ac.threshold, ac.floor, ac.dilate) != 0;
	const unsigned long long mask = __ballot(keep);
	if (lane == 0) { act_out[blockIdx.x * (JP_BLOCK / 64) + wave] = mask; s_cnt[wave] = (unsigned int)__popcll(mask); }
	__syncthreads();
	if (threadIdx.x == 0) { unsigned int t = 0; for (int w = 0; w < JP_BLOCK / 64; w++) t += s_cnt[w]; blk_tot[blockIdx.x] = t; }
}

__global__ void __launch_bounds__(JP_BLOCK) k_adapt_scan(const unsigned int* __restrict__ blk_tot, unsigned int* __restrict__ blk_off, unsigned int nblocks, unsigned int* n_active_host)
{
	__shared__ unsigned int s_run[JP_BLOCK];
	const unsigned int per = (nblocks + JP_BLOCK - 1) / JP_BLOCK;
	const unsigned int i0 = min(threadIdx.x * per, nblocks), i1 = min(i0 + per, nblocks);
	unsigned int t = 0;
	for (unsigned int i = i0; i < i1; i++) t += blk_tot[i];
	s_run[threadIdx.x] = t;
	__syncthreads();
	for (unsigned int d = 1; d < JP_BLOCK; d <<= 1)                   // inclusive scan of the run totals
	{
		const unsigned int v = threadIdx.x >= d ? s_run[threadIdx.x - d] : 0u;
		__syncthreads();
		s_run[threadIdx.x] += v;
		__syncthreads();
	}
	unsigned int off = s_run[threadIdx.x] - t;
	for (unsigned int i = i0; i < i1; i++) { blk_off[i] = off; off += blk_tot[i]; }
	if (threadIdx.x == JP_BLOCK - 1) { *n_active_host = s_run[JP_BLOCK - 1]; __threadfence_system(); }
}

__global__ void __launch_bounds__(JP_BLOCK) k_adapt_compact(int npix, const unsigned long long* __restrict__ act, const unsigned int* __restrict__ blk_off, unsigned int* __restrict__ list)
{
	__shared__ unsigned int s_cnt[JP_BLOCK / 64];
	const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const unsigned long long mask = act[blockIdx.x * (JP_BLOCK / 64) + wave];
	if (lane == 0) s_cnt[wave] = (unsigned int)__popcll(mask);
	__syncthreads();
	unsigned int base = blk_off[blockIdx.x];
	for (unsigned int w = 0; w < wave; w++) base += s_cnt[w];
	const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
	const unsigned int p = blockIdx.x * JP_BLOCK + threadIdx.x;
	if (((mask >> lane) & 1ull) && p < (unsigned int)npix) list[base + rank] = p;
}

// k_adapt_finish: the film, the counts and the variance of the shard's pixels in the film's pixel layout (each plane may be null; all are zero before)
__global__ void __launch_bounds__(JP_BLOCK) k_adapt_finish(RenderConst rc, const float4* __restrict__ sum, const float2* __restrict__ mom, float* film, int* counts, float* variance, int hdr)
{
	for (int pix = blockIdx.x * JP_BLOCK + threadIdx.x; pix < rc.npix; pix += gridDim.x * JP_BLOCK)
	{
		const float4 a = sum[pix];
		const int n = __float_as_int(a.w);
		const float s3[3] = { a.x, a.y, a.z };
		float rgb[3], v;
		jp_adapt_finish(s3, mom[pix].y, n, hdr, rgb, &v);
		int x, y; pixel_of(rc, pix, x, y);
		const size_t o = (size_t)y * rc.width + x;
		if (film) { film[3 * o] = rgb[0]; film[3 * o + 1] = rgb[1]; film[3 * o + 2] = rgb[2]; }
		if (counts) counts[o] = n;
		if (variance) variance[o] = v;
	}
}
#endif // JP_ADAPTIVE_DEVICE_PART

#if defined(JP_ADAPTIVE_RUNTIME) && !defined(JP_ADAPTIVE_RUNTIME_PART)
#define JP_ADAPTIVE_RUNTIME_PART

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace
{
int adaptive_check_status(const JpAdaptive* a)
{
	if (!a) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: null JpAdaptive");
	switch (jp_adapt_check(a))
	{
	case 0: return JP_OK;
	case 1: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: set JpAdaptive.struct_bytes to sizeof(JpAdaptive)");
	case 2: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: min_spp must be >= 2 (the sample variance of one sample is undefined)");
	case 3: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: step_spp must be >= 1");
	case 4: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: max_spp must be >= min_spp (0: JpRenderParams.spp)");
	case 5: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: threshold must be finite and >= 0");
	case 6: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: floor must be finite and >= 0 (0: the default, 1e-3)");
	default: return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: dilate must be 0 or 1");
	}
}
// ... and with max_spp resolved (spp: what stands in for 0)
int adaptive_resolve(const JpAdaptive* a, int spp, JpAdaptive& r)
{
	if (const int e = adaptive_check_status(a); e != JP_OK) return e;
	r = *a; r.struct_bytes = (int32_t)sizeof(JpAdaptive);
	if (r.max_spp == 0) r.max_spp = spp;
	if (r.max_spp < r.min_spp) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: max_spp must be >= min_spp (0: JpRenderParams.spp)");
	r.floor = jp_adapt_floor(r.floor);
	return JP_OK;
}

// The per-pixel state of one call and the selection's launches: what the render and the probe share.  Freed when the call returns (the caller waits for the stream).
struct AdaptState
{
	DevBuf b_sum, b_mom, b_act[2], b_tot, b_off, b_list; PinnedBuf word;
	float4* sum = nullptr; float2* mom = nullptr; unsigned long long* act[2] = { nullptr, nullptr }; unsigned int *tot = nullptr, *off = nullptr, *list = nullptr;
	unsigned int nblocks = 0; int cur = 0; bool have_list = false;
	long long bytes() const { return (long long)(b_sum.bytes() + b_mom.bytes() + b_act[0].bytes() + b_act[1].bytes() + b_tot.bytes() + b_off.bytes() + b_list.bytes()); }
	const unsigned int* list_or_null() const { return have_list ? list : nullptr; }

	int begin(JpContext* c, long long npix)
	{
		nblocks = (unsigned int)((npix + JP_BLOCK - 1) / JP_BLOCK);
		const size_t nmask = (size_t)nblocks * (JP_BLOCK / 64) * sizeof(unsigned long long);
		HIP_TRY(reserve(b_sum, sum, (size_t)npix * sizeof(float4))); HIP_TRY(reserve(b_mom, mom, (size_t)npix * sizeof(float2)));
		HIP_TRY(reserve(b_act[0], act[0], nmask)); HIP_TRY(reserve(b_act[1], act[1], nmask));
		HIP_TRY(reserve(b_tot, tot, (size_t)nblocks * 4)); HIP_TRY(reserve(b_off, off, (size_t)nblocks * 4)); HIP_TRY(reserve(b_list, list, (size_t)npix * 4));
		if (word.reserve(sizeof(unsigned int)) != hipSuccess) return fail(JP_ERR_DEVICE, "jp_render_adaptive: no pinned memory for the active count");
		HIP_TRY(hipMemsetAsync(sum, 0, (size_t)npix * sizeof(float4), c->stream)); HIP_TRY(hipMemsetAsync(mom, 0, (size_t)npix * sizeof(float2), c->stream));
		HIP_TRY(hipMemsetAsync(act[0], 0xff, nmask, c->stream));            // everyone is active (k_adapt_select looks at pixels below npix only)
		cur = 0; have_list = false;
		return JP_OK;
	}
	void resolve(JpContext* c, const float4* lacc, unsigned int n_act, int s0, int sbatch, float sample_clamp)
	{
		Stamper t(c, CLS_ADAPT_RESOLVE);
		const dim3 grid((unsigned int)std::min<long long>(c->n_cus * 8, ((long long)n_act + JP_BLOCK - 1) / JP_BLOCK));
		hipLaunchKernelGGL(k_resolve_list, grid, dim3(JP_BLOCK), 0, c->stream, lacc, n_act, list_or_null(), s0, sbatch, sum, mom, sample_clamp);
	}
	// the test after a pass: the next list and its length (waits for the stream: the one word the host reads per pass)
	int select(JpContext* c, const AdaptConst& ac, unsigned int& n_act)
	{
		{
			Stamper t(c, CLS_ADAPT_SELECT);
			hipLaunchKernelGGL(k_adapt_select, dim3(nblocks), dim3(JP_BLOCK), 0, c->stream, ac, (const float4*)sum, (const float2*)mom, (const unsigned long long*)act[cur], act[cur ^ 1], tot);
			hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(JP_BLOCK), 0, c->stream, (const unsigned int*)tot, off, nblocks, word.get<unsigned int>());
			hipLaunchKernelGGL(k_adapt_compact, dim3(nblocks), dim3(JP_BLOCK), 0, c->stream, ac.npix, (const unsigned long long*)act[cur ^ 1], (const unsigned int*)off, list);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(c->stream));
		n_act = *word.get<volatile unsigned int>();
		if (n_act > (unsigned int)ac.npix) return fail(JP_ERR_DEVICE, "jp_render_adaptive: the selection returned more pixels than the shard has");
		cur ^= 1; have_list = true;
		return JP_OK;
	}
	void finish(JpContext* c, const RenderConst& rc, float* film, int* counts, float* variance, int hdr)
	{
		const dim3 grid((unsigned int)std::min<long long>(c->n_cus * 8, ((long long)rc.npix + JP_BLOCK - 1) / JP_BLOCK));
		hipLaunchKernelGGL(k_adapt_finish, grid, dim3(JP_BLOCK), 0, c->stream, rc, (const float4*)sum, (const float2*)mom, film, counts, variance, hdr);
	}
};

void adaptive_note(JpContext* c, const JpAdaptive& a)
{
	JpAdaptiveInfo& i = c->ad_info; std::memset(&i, 0, sizeof(i));
	i.adaptive_last_render = 1; i.min_spp = a.min_spp; i.step_spp = a.step_spp; i.max_spp = a.max_spp; i.dilate = a.dilate; i.threshold = a.threshold;
	for (int k = 0; k < 16; k++) i.active_after[k] = -1;
}

AdaptConst adapt_const(const JpAdaptive& a, const JpAdaptShard& sh, long long npix)
{
	AdaptConst ac; ac.sh = sh; ac.npix = (int)npix; ac.threshold = a.threshold; ac.floor = a.floor; ac.dilate = a.dilate;
	return ac;
}

// The driver loop: render_one's frame (one lane: batch sizing, queue set, plan, kernel selectors, the launches of a bounce) around the list twins.  The first pass
// is uniform (identity list); every pass of n_act pixels x ns samples is cut into batches of whole samples that fit the queue budget, and the queue geometry
// (G regions of R slots) follows the batch, as it follows npix x sbatch in render_one.
int adaptive_render(JpContext* c, const JpRenderParams* rp, const JpAdaptive* ad, float* film_dev, int* counts_dev, float* var_dev)
{
	if (!c || !rp || (!film_dev && !counts_dev && !var_dev)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: null argument");
	Shard sh;
	if (const int e = shard_of(rp, sh); e != JP_OK) return e;
	JpAdaptive a;
	if (const int e = adaptive_resolve(ad, rp->spp, a); e != JP_OK) return e;
	if (rp->integrator != JP_INTEGRATOR_PATH) return fail(JP_ERR_UNSUPPORTED, "jp_render_adaptive: the path integrator only (the Whitted and debug integrators take jp_render)");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_render_adaptive: no scene uploaded");
	if (c->estimator == JP_ESTIMATOR_MIS && !c->plan.pick)
		return fail(JP_ERR_UNSUPPORTED, "jp_render_adaptive: JP_ESTIMATOR_MIS needs a scene uploaded with JP_LIGHTS_POWER_ONE (jp_set_light_sampling): the light strategy's pdf comes from the light table");
	const ScenePlan& p = c->plan; DevCounters* const d_cnt = c->cnt.get<DevCounters>();
	HIP_TRY(hipSetDevice(c->device));
	const long long npix = (long long)sh.local_rows * rp->width;
	if (npix > (1 << 24)) return fail(JP_ERR_UNSUPPORTED, "jp_render_adaptive: more than 2^24 pixels per shard");

	// what render_impl notes of a render (JpBuildInfo, the *_last_render fields): one lane, the per-bounce launches
	c->last_hdr = c->film_on ? 1 : 0; c->last_var = 0;
	if (c->var_mom || (!c->lanes.empty() && c->lanes[0]->var_mom)) { HIP_TRY(hipStreamSynchronize(c->stream)); c->var_mom.reset(); for (JpContext* l : c->lanes) l->var_mom.reset(); }
	c->last_lanes = 1; c->last_fused = 0;
	c->last_textured = p.textured ? 1 : 0; c->last_picked = p.pick ? 1 : 0; c->last_mapped = p.env ? 1 : 0; c->last_mis = c->estimator == JP_ESTIMATOR_MIS ? 1 : 0;
	c->last_smooth = p.smooth ? 1 : 0; c->last_nmapped = p.mapped ? 1 : 0; c->last_sampled = ((p.textured && p.sm.tex) || (p.mapped && p.sm.map)) ? 1 : 0;
	c->last_mip = p.textured && p.mip_on > 0 ? 1 : 0; c->last_proc = p.textured && p.proc_on > 0 ? 1 : 0; c->last_lens = c->lens_on ? 1 : 0;
	c->last_proj = 0; c->last_proj_gamma0 = 0.f;
	adaptive_note(c, a);

	const size_t nfilm = (size_t)rp->width * rp->height;
	HIP_TRY(hipEventRecord(c->ev0, c->stream));
	if (film_dev) HIP_TRY(hipMemsetAsync(film_dev, 0, sizeof(float) * 3 * nfilm, c->stream));
	if (counts_dev) HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int) * nfilm, c->stream));
	if (var_dev) HIP_TRY(hipMemsetAsync(var_dev, 0, sizeof(float) * nfilm, c->stream));
	HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(DevCounters), c->stream));
	c->evused = 0; c->stamps.clear();
	unsigned long long samples = 0;
	AdaptState st;
	if (npix > 0)
	{
		if (const int e = st.begin(c, npix); e != JP_OK) return e;
		c->ad_info.state_bytes_device = st.bytes();
		const int slot_bits = p.n_planes <= 31 ? 27 : 24;
		const unsigned int PMAX = slot_bits == 27 ? (1u << 26) : (1u << 24);
		size_t freeB = 0, totalB = 0; hipMemGetInfo(&freeB, &totalB);
		const bool smooth = p.smooth, tex = p.textured, mis = c->estimator == JP_ESTIMATOR_MIS;
		const size_t per = 136 + 32 * (size_t)p.n_planes + (smooth ? 16 : 0);
		size_t budget = std::min<size_t>((size_t)24 << 30, (freeB + (c->cap ? (size_t)c->cap * (136 + 32 * (size_t)c->planes_alloc) : 0)) / 2);
		if (c->opt.max_slots > 0) budget = std::min<size_t>(budget, (size_t)c->opt.max_slots * per);
		const unsigned int pcap = (unsigned int)std::min<size_t>(PMAX, std::max<size_t>((size_t)npix, budget / per));

		RenderConst rc; rc.width = rp->width; rc.height = rp->height; rc.spp = a.max_spp; rc.max_depth = rp->max_depth; rc.seed = rp->seed;
		rc.band_rows = sh.band; rc.shard_index = sh.index; rc.shard_count = sh.count; rc.npix = (int)npix; rc.local_rows = sh.local_rows; rc.n_planes = p.n_planes;
		rc.lane_index = 0; rc.lane_count = 1; rc.lane_rows = 4; rc.class_mask = p.class_mask; rc.sampler_debug = rp->sampler_mode == JP_SAMPLER_DEBUG ? 1 : 0;
		rc.slot_bits = slot_bits; rc.tiled = 0; rc.compact = 0; rc.s0 = 0; rc.sbatch = 0;
		const bool generic = c->opt.reserved[0] == 1;
		const ExtendLaunch ek = extend_kernel(p, generic);
		JpLensPlan lp;
		if (const int e = lens_plan_of(c, lp); e != JP_OK) return e;
		JpProjectionPlan pp;
		if (const int e = proj_plan_of(c, pp); e != JP_OK) return e;
		if (c->proj_on) { c->last_proj = 1; c->last_proj_gamma0 = pp.gamma0; }
		const JpAdaptShard ash = { rp->width, rp->height, sh.band, sh.index, sh.count };
		const AdaptConst ac = adapt_const(a, ash, npix);
		const float sample_clamp = c->film_on ? c->film_state.sample_clamp : 0.f;

		unsigned int n_act = (unsigned int)npix;
		int n_cur = 0, ns = a.min_spp;
		while (n_act > 0)
		{
			// ---- the pass: n_act pixels x ns samples from sample index n_cur, in batches of sbatch whole samples ----
			// (when the queue allocation fails -- another process took the memory in between -- the batch is halved and tried again, as in render_one)
			int sbatch = 1; unsigned int G = 1, R = JP_BLOCK, cap = 0;
			size_t pass_cap = pcap;
			for (int attempt = 0;; attempt++)
			{
				sbatch = (int)std::max<long long>(1, std::min<long long>(ns, (long long)(pass_cap / n_act)));
				{ const int nb = (ns + sbatch - 1) / sbatch; sbatch = (ns + nb - 1) / nb; }
				const unsigned int P = (unsigned int)sbatch * n_act;        // (<= PMAX: n_act <= npix <= pcap <= PMAX)
				const unsigned int nchunks = (P + JP_BLOCK - 1) / JP_BLOCK;
				G = std::max(1u, std::min(nchunks, (unsigned int)(c->n_cus * c->blocks_per_cu)));
				G = std::max(G, (nchunks + JP_SHADE_TILE / JP_BLOCK - 1) / (JP_SHADE_TILE / JP_BLOCK));
				R = ((nchunks + G - 1) / G) * JP_BLOCK; cap = G * R;
				const int e = ensure_queues(c, cap, p.n_planes, G);
				if (e == JP_OK) break;
				if (sbatch <= 1 || attempt >= 6) return e;                 // one sample per active pixel does not fit either: out of device memory
				pass_cap = (size_t)(sbatch / 2) * n_act;                   // half the batch
			}
			c->q.cap = cap; c->q.R = R;
			if (tex) if (const int e = reserve_idle(c, c->side, (size_t)cap * sizeof(unsigned int)); e != JP_OK) return e;
			TexView tv = p.tv; tv.side = c->side.get<unsigned int>();
			MipView mv_cone = {};
			if (tex && (p.mip_on > 0 || p.proc_aa > 0)) { mv_cone = p.mv; if (const int e = ensure_cone(c, cap, mv_cone); e != JP_OK) return e; }
			if (c->proj_on) mv_cone.gamma0 = pp.gamma0;
			MisView mv = {};
			if (mis) if (const int e = ensure_mis_side(c, cap, mv); e != JP_OK) return e;
			NormView nv = p.nv;
			if (smooth) if (const int e = ensure_normal_side(c, cap, nv); e != JP_OK) return e;
			if (const int e = reserve_idle(c, c->spill, spill_need(p, p.persist ? deepest_walk(p) : 0, G) * sizeof(int)); e != JP_OK) return e;
			int* const d_spill = c->spill.get<int>();
			const int grid = (int)G;
			const ShadowLaunch sk = shadow_kernel(p, R, generic);
			const ShadeLaunch shade = shade_launch(shade_choice(p, tex, mis, smooth, generic), ShadeViews(tv, p.pv, p.ev, mv, nv));
			for (int b0 = 0; b0 < ns; b0 += sbatch)
			{
				rc.s0 = n_cur + b0; rc.sbatch = std::min(sbatch, ns - b0);
				{
					Stamper t(c, CLS_OTHER);
					if (c->proj_on) hipLaunchKernelGGL(k_raygen_list_proj, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, pp, st.list_or_null(), n_act);
					else if (c->lens_on) hipLaunchKernelGGL(k_raygen_list<true>, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, lp, st.list_or_null(), n_act);
					else hipLaunchKernelGGL(k_raygen_list<false>, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, rc, d_cnt, NoLens(), st.list_or_null(), n_act);
				}
				if (const int e = launch_bounces(c, rp, p, rc, grid, BounceLaunch{ ek, sk, shade, tex, smooth, tv, mv_cone, nv, d_spill, d_cnt }); e != JP_OK) return e;
				st.resolve(c, c->q.lacc, n_act, rc.s0, rc.sbatch, sample_clamp);
				samples += (unsigned long long)rc.sbatch * n_act;
			}
			HIP_TRY(hipGetLastError());
			n_cur += ns; c->ad_info.passes++;
			if (n_cur >= a.max_spp) break;
			if (const int e = st.select(c, ac, n_act); e != JP_OK) return e;
			if (c->ad_info.passes <= 16) c->ad_info.active_after[c->ad_info.passes - 1] = (int32_t)n_act;
			ns = jp_adapt_next(n_cur, a.step_spp, a.max_spp);
		}
		st.finish(c, rc, film_dev, counts_dev, var_dev, c->film_on ? c->film_state.hdr : 0);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipEventRecord(c->ev1, c->stream));
	c->own_samples = samples; c->ad_info.samples_traced = (int64_t)samples;
	HIP_TRY(hipStreamSynchronize(c->stream));                          // the state goes when this function returns
	return JP_OK;
}
}

extern "C" {

int jp_check_adaptive(const JpAdaptive* a) { return adaptive_check_status(a); }

int jp_render_adaptive_device(JpContext* c, const JpRenderParams* rp, const JpAdaptive* ad, void* film_dev, void* counts_dev, void* variance_dev, int)
{
	if (rp && rp->width > 0 && rp->height > 0)
	{
		const size_t n = (size_t)rp->width * rp->height;
		if ((film_dev && counts_dev && overlaps(film_dev, n * 12, counts_dev, n * 4)) || (film_dev && variance_dev && overlaps(film_dev, n * 12, variance_dev, n * 4))
		    || (counts_dev && variance_dev && overlaps(counts_dev, n * 4, variance_dev, n * 4)))
			return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: the output planes overlap");
	}
	return adaptive_render(c, rp, ad, (float*)film_dev, (int*)counts_dev, (float*)variance_dev);
}

int jp_render_adaptive(JpContext* c, const JpRenderParams* rp, const JpAdaptive* ad, float* film_host, int32_t* counts_host, float* variance_host)
{
	if (!c || !rp || (!film_host && !counts_host && !variance_host)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: null argument");
	if (rp->width <= 0 || rp->height <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_adaptive: bad width/height");
	HIP_TRY(hipSetDevice(c->device));
	const size_t npix = (size_t)rp->width * rp->height;
	if (const int e = ensure_film(c, 3 * npix); e != JP_OK) return e;
	if (const int e = reserve_idle(c, c->var_plane, npix * sizeof(float)); e != JP_OK) return e;
	DevBuf b_cnt; int* d_cnt;                                          // the count plane: per-call scratch
	HIP_TRY(reserve(b_cnt, d_cnt, npix * sizeof(int)));
	float* const d_film = c->film.get<float>(); float* const d_var = c->var_plane.get<float>();
	if (const int e = adaptive_render(c, rp, ad, d_film, d_cnt, d_var); e != JP_OK) return e;
	if (film_host) HIP_TRY(hipMemcpyAsync(film_host, d_film, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (counts_host) HIP_TRY(hipMemcpyAsync(counts_host, d_cnt, npix * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	if (variance_host) HIP_TRY(hipMemcpyAsync(variance_host, d_var, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

static int adaptive_samples_check(const char* who, const JpFilm* f, const JpAdaptive* ad, int32_t width, int32_t height, const float* samples, const void* film, const void* counts, const void* variance, JpAdaptive& a)
{
	if (const int e = adaptive_resolve(ad, 0, a); e != JP_OK) return e;      // (max_spp 0 has nothing to stand in for it here: refused as max_spp < min_spp)
	if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 24)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": bad width/height (at most 2^24 pixels)");
	if ((long long)width * height * a.max_spp > (1ll << 30)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": at most 2^30 samples");
	if (!samples || (!film && !counts && !variance)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
	if (f) if (const int e = film_check_status(f); e != JP_OK) return e;
	return JP_OK;
}

int jp_adaptive_samples(const JpFilm* f, const JpAdaptive* ad, int32_t width, int32_t height, const float* samples_rgb, float* film, int32_t* counts, float* variance)
{
	JpAdaptive a;
	if (const int e = adaptive_samples_check("jp_adaptive_samples", f, ad, width, height, samples_rgb, film, counts, variance, a); e != JP_OK) return e;
	const JpAdaptShard sh = { width, height, height, 0, 1 };
	std::vector<float> scratch((size_t)jp_adapt_scratch_floats((int64_t)width * height));
	jp_adapt_samples(f ? f->sample_clamp : 0.f, f ? f->hdr : 0, &a, &sh, samples_rgb, scratch.data(), film, counts, variance);
	return JP_OK;
}

int jp_adaptive_probe(JpContext* c, const JpFilm* f, const JpAdaptive* ad, int32_t width, int32_t height, const float* samples_rgb, float* film, int32_t* counts, float* variance)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_adaptive_probe: null context");
	JpAdaptive a;
	if (const int e = adaptive_samples_check("jp_adaptive_probe", f, ad, width, height, samples_rgb, film, counts, variance, a); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const long long npix = (long long)width * height;
	const size_t nsamp = (size_t)a.max_spp * (size_t)npix * 3;
	const int smax_ = std::max(a.min_spp, a.step_spp);
	DevBuf b_s, b_l, b_f, b_c, b_v; float* d_s; float4* d_l; float* d_f; int* d_c; float* d_v;   // per-call scratch: freed on every return
	HIP_TRY(reserve(b_s, d_s, nsamp * sizeof(float))); HIP_TRY(reserve(b_l, d_l, (size_t)npix * std::min(smax_, a.max_spp) * sizeof(float4)));
	HIP_TRY(reserve(b_f, d_f, (size_t)npix * 12)); HIP_TRY(reserve(b_c, d_c, (size_t)npix * 4)); HIP_TRY(reserve(b_v, d_v, (size_t)npix * 4));
	HIP_TRY(hipMemcpyAsync(d_s, samples_rgb, nsamp * sizeof(float), hipMemcpyHostToDevice, c->stream));
	adaptive_note(c, a);
	c->evused = 0; c->stamps.clear();
	AdaptState st;
	if (const int e = st.begin(c, npix); e != JP_OK) return e;
	c->ad_info.state_bytes_device = st.bytes();
	const JpAdaptShard sh = { width, height, height, 0, 1 };
	const AdaptConst ac = adapt_const(a, sh, npix);
	RenderConst rc; std::memset(&rc, 0, sizeof(rc));
	rc.width = width; rc.height = height; rc.band_rows = height; rc.shard_index = 0; rc.shard_count = 1; rc.npix = (int)npix; rc.local_rows = height; rc.lane_count = 1; rc.lane_rows = 4;
	unsigned int n_act = (unsigned int)npix; int n_cur = 0, ns = a.min_spp; unsigned long long samples = 0;
	while (n_act > 0)
	{
		const size_t total = (size_t)n_act * ns;
		hipLaunchKernelGGL(k_adapt_probe_fill, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (total + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream,
		                   d_l, (const float*)d_s, (unsigned int)npix, n_act, st.list_or_null(), n_cur, ns);
		st.resolve(c, d_l, n_act, n_cur, ns, f ? f->sample_clamp : 0.f);
		HIP_TRY(hipGetLastError());
		samples += total; n_cur += ns; c->ad_info.passes++;
		if (n_cur >= a.max_spp) break;
		if (const int e = st.select(c, ac, n_act); e != JP_OK) return e;
		if (c->ad_info.passes <= 16) c->ad_info.active_after[c->ad_info.passes - 1] = (int32_t)n_act;
		ns = jp_adapt_next(n_cur, a.step_spp, a.max_spp);
	}
	HIP_TRY(hipMemsetAsync(d_f, 0, (size_t)npix * 12, c->stream)); HIP_TRY(hipMemsetAsync(d_c, 0, (size_t)npix * 4, c->stream)); HIP_TRY(hipMemsetAsync(d_v, 0, (size_t)npix * 4, c->stream));
	st.finish(c, rc, d_f, d_c, d_v, f ? f->hdr : 0);
	HIP_TRY(hipGetLastError());
	c->ad_info.samples_traced = (int64_t)samples;
	if (film) HIP_TRY(hipMemcpyAsync(film, d_f, (size_t)npix * 12, hipMemcpyDeviceToHost, c->stream));
	if (counts) HIP_TRY(hipMemcpyAsync(counts, d_c, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
	if (variance) HIP_TRY(hipMemcpyAsync(variance, d_v, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_get_adaptive_info(JpContext* c, JpAdaptiveInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_adaptive_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_adaptive_info: set JpAdaptiveInfo.struct_bytes to sizeof(JpAdaptiveInfo)");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	JpAdaptiveInfo i; std::memset(&i, 0, sizeof(i));
	if (c->ad_info.adaptive_last_render)
	{
		i = c->ad_info;
		for (const JpContext::Stamp& s : c->stamps)
		{
			if (s.cls != CLS_ADAPT_SELECT && s.cls != CLS_ADAPT_RESOLVE) continue;
			float t = 0.f; if (hipEventElapsedTime(&t, c->evpool[s.a], c->evpool[s.b]) != hipSuccess) continue;
			(s.cls == CLS_ADAPT_SELECT ? i.select_ms : i.resolve_ms) += t;
		}
	}
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

} // extern "C"

#endif // JP_ADAPTIVE_RUNTIME
