// jet-pbrt_amd/csrc/jp_variance.h -- the per-pixel variance of the film and the variance-guided a-trous filter (include/jetpbrt_amd.h "Variance", DESIGN.md
// "Variance").  The moments' definition is include/jp_variance.h, shared with the host.  Two parts, like jp_film.h: part 1 (after k_resolve_film in
// jp_kernels.hip: k_resolve_var, the third twin launch_resolve picks, and k_var_probe) and, with JP_VARIANCE_RUNTIME defined, part 2 LAST: k_atrous_v_pack,
// k_atrous_v and the entry points.  Nothing runs unless one of the new entry points is called: every kernel above compiles to the instructions it compiled to
// without this file (tools/asm_kernel_diff.py).
#ifndef JP_VARIANCE_DEVICE_PART
#define JP_VARIANCE_DEVICE_PART
#include "../../include/jp_variance.h"

// ---------------------------------------------------------------------------------------------------------------------
// k_resolve_var: k_resolve_film's twin while a variance render runs (jp_render_variance*): the same sum in the same order with the same hdr and sample_clamp
// handling (no film state in force: hdr = 0, sample_clamp = 0 -- k_resolve's film), and the moments of the samples' luminances (include/jp_variance.h) in
// mom[pix] = (mean, m2) across batches; the last batch writes the variance of the pixel's mean onto the (zero) variance plane, in the film's pixel layout.
// A kernel of its own text, like k_resolve_film: the other two keep their instruction streams.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JP_BLOCK) k_resolve_var(Queues q, RenderConst rc, float4* pix_acc, float* film, float2* mom, float* variance, int first, int last, int hdr, float sample_clamp)
{
	const float ratio = 1.0f / (float)rc.spp;
	for (int pix = blockIdx.x * JP_BLOCK + threadIdx.x; pix < rc.npix; pix += gridDim.x * JP_BLOCK)
	{
		V3 L = mk(0, 0, 0); float mean = 0.f, m2 = 0.f;
		if (!first) { const float4 a = pix_acc[pix]; L = mk(a.x, a.y, a.z); const float2 m = mom[pix]; mean = m.x; m2 = m.y; }
		for (int s = 0; s < rc.sbatch; s++)
		{
			float4 l = q.lacc[(size_t)s * rc.npix + pix];
			if (sample_clamp > 0.f) jp_film_clamp_sample(sample_clamp, &l.x, &l.y, &l.z);
			L = L + mk(l.x, l.y, l.z) * ratio;
			jp_var_step(&mean, &m2, jp_var_luminance(l.x, l.y, l.z), rc.s0 + s + 1);
		}
		if (!last) { pix_acc[pix] = make_float4(L.x, L.y, L.z, 0.f); mom[pix] = make_float2(mean, m2); }
		else
		{
			int x, y; pixel_of(rc, pix, x, y);
			float* o = film + 3 * ((size_t)y * rc.width + x);
			if (hdr) { o[0] = 0.f + smax(L.x, 0.f); o[1] = 0.f + smax(L.y, 0.f); o[2] = 0.f + smax(L.z, 0.f); }
			else { o[0] = 0.f + clampf(L.x, 0.f, 1.f); o[1] = 0.f + clampf(L.y, 0.f, 1.f); o[2] = 0.f + clampf(L.z, 0.f, 1.f); }
			variance[(size_t)y * rc.width + x] = jp_var_of_mean(m2, rc.spp);
		}
	}
}

// k_var_probe (jp_variance_probe): the moments of k_resolve_var on caller-supplied samples [spp][n][3], one launch per batch of sbatch samples from s0
__global__ void __launch_bounds__(JP_BLOCK) k_var_probe(long long n, int spp, int s0, int sbatch, const float* __restrict__ samples, float2* mom, float* __restrict__ variance, float sample_clamp)
{
	for (long long p = (long long)blockIdx.x * JP_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * JP_BLOCK)
	{
		float mean = 0.f, m2 = 0.f;
		if (s0 > 0) { const float2 m = mom[p]; mean = m.x; m2 = m.y; }
		for (int s = s0; s < s0 + sbatch; s++)
		{
			const float* l = samples + 3 * ((long long)s * n + p);
			float r = l[0], g = l[1], b = l[2];
			if (sample_clamp > 0.f) jp_film_clamp_sample(sample_clamp, &r, &g, &b);
			jp_var_step(&mean, &m2, jp_var_luminance(r, g, b), s + 1);
		}
		if (s0 + sbatch < spp) mom[p] = make_float2(mean, m2);
		else variance[p] = jp_var_of_mean(m2, spp);
	}
}
#endif // JP_VARIANCE_DEVICE_PART

#if defined(JP_VARIANCE_RUNTIME) && !defined(JP_VARIANCE_RUNTIME_PART)
#define JP_VARIANCE_RUNTIME_PART

// ---------------------------------------------------------------------------------------------------------------------
// k_atrous_v: one iteration of the variance-guided filter (INTEGRATION.md "Variance-guided filter").  k_atrous's records and tile; the variance of a pixel's
// (demodulated) colour rides in the .w of its normal record, which k_atrous leaves unused: a tap still is two dwordx4 loads, and the normal records ping-pong
// with the colours (16 bytes more written per pixel and iteration).  Per pixel first g, the 3 x 3 binomial of the neighbours' variances at distance 1 (nine
// dword loads next to the centre's cache lines), which scales the colour edge-stop; then the 25 taps, which also carry the variance: vnum += w^2 v_q.
// The last iteration re-modulates, clamps (hdr: max(., 0)) and writes the film layout and the variance plane.
// ---------------------------------------------------------------------------------------------------------------------
struct AtrousVConst
{
	int width, height, step;
	float sc2, kn, kz;
	int hdr;
};

__device__ __forceinline__ float atrous_v_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ void __launch_bounds__(JP_BLOCK) k_atrous_v_pack(int npix, const float* __restrict__ film, const float* __restrict__ albedo, const float* __restrict__ normal,
                                                             const float* __restrict__ dist, const float* __restrict__ variance, float4* __restrict__ cz, float4* __restrict__ nv)
{
	for (int p = blockIdx.x * JP_BLOCK + threadIdx.x; p < npix; p += gridDim.x * JP_BLOCK)
	{
		float ar = 1.f, ag = 1.f, ab = 1.f;
		if (albedo) { ar = smax(albedo[3 * p], 0.001f); ag = smax(albedo[3 * p + 1], 0.001f); ab = smax(albedo[3 * p + 2], 0.001f); }
		const float aY = atrous_v_lum(ar, ag, ab);
		const float v = variance[p];
		const float vin = v > 0.f ? (v < 1e30f ? v : 1e30f) : 0.f;          // NaN and negative inputs: 0
		cz[p] = make_float4(film[3 * p] / ar, film[3 * p + 1] / ag, film[3 * p + 2] / ab, dist[p]);
		nv[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], vin / (aY * aY));
	}
}

template <bool kLast>
__global__ void __launch_bounds__(JP_BLOCK) k_atrous_v(AtrousVConst ac, const float4* __restrict__ cz, const float4* __restrict__ nv, float4* __restrict__ cz_out, float4* __restrict__ nv_out,
                                                        const float* __restrict__ albedo, float* __restrict__ out, float* __restrict__ var_out)
{
	const int x = blockIdx.x * JP_ATROUS_TW + (threadIdx.x & (JP_ATROUS_TW - 1)), y = blockIdx.y * JP_ATROUS_TH + (threadIdx.x / JP_ATROUS_TW);
	if (x >= ac.width || y >= ac.height) return;
	const int p = y * ac.width + x;
	const float4 cp = cz[p], np = nv[p];
	float gs = 0.f, ks = 0.f;
	#pragma unroll
	for (int dy = -1; dy <= 1; dy++)
	{
		const int qy = y + dy;
		if (qy < 0 || qy >= ac.height) continue;
		const float ky = dy == 0 ? 0.5f : 0.25f;
		#pragma unroll
		for (int dx = -1; dx <= 1; dx++)
		{
			const int qx = x + dx;
			if (qx < 0 || qx >= ac.width) continue;
			const float k3 = ky * (dx == 0 ? 0.5f : 0.25f);
			gs += k3 * nv[qy * ac.width + qx].w; ks += k3;
		}
	}
	const float kc = 1.0f / (ac.sc2 * (gs / ks) + 1e-8f);
	float nr_ = 0.f, ng_ = 0.f, nb_ = 0.f, den = 0.f, vnum = 0.f;
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
			const float4 cq = cz[q], nq = nv[q];
			const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
			const float dc = (dr * dr + dg * dg) + db * db;
			const float ex = np.x - nq.x, ey = np.y - nq.y, ez = np.z - nq.z;
			const float dn = (ex * ex + ey * ey) + ez * ez;
			const float m = smax(smax(cp.w, cq.w), 1e-20f);
			const float rz = (cp.w - cq.w) / m;
			const float dz = rz * rz;
			const float w = hh / (((1.f + dc * kc) * (1.f + dn * ac.kn)) * (1.f + dz * ac.kz));
			nr_ += w * cq.x; ng_ += w * cq.y; nb_ += w * cq.z; den += w; vnum += (w * w) * nq.w;
		}
	}
	const float r = nr_ / den, g = ng_ / den, b = nb_ / den, vn = vnum / (den * den);   // (the centre tap is always there: den >= 9/64)
	if (!kLast) { cz_out[p] = make_float4(r, g, b, cp.w); nv_out[p] = make_float4(np.x, np.y, np.z, vn); }
	else
	{
		float ar = 1.f, ag = 1.f, ab = 1.f;
		if (albedo) { ar = smax(albedo[3 * p], 0.001f); ag = smax(albedo[3 * p + 1], 0.001f); ab = smax(albedo[3 * p + 2], 0.001f); }
		if (ac.hdr) { out[3 * p] = smax(r * ar, 0.f); out[3 * p + 1] = smax(g * ag, 0.f); out[3 * p + 2] = smax(b * ab, 0.f); }
		else { out[3 * p] = clampf(r * ar, 0.f, 1.f); out[3 * p + 1] = clampf(g * ag, 0.f, 1.f); out[3 * p + 2] = clampf(b * ab, 0.f, 1.f); }
		if (var_out) { const float aY = atrous_v_lum(ar, ag, ab); var_out[p] = vn * (aY * aY); }
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace
{
#define JP_DENOISE_V_SIGMA_COLOR 8.0f

// the moments live while a variance render runs: freed by the entry point once its stream is idle (a call with sync = 0: by the next jp_render*)
void release_moments(JpContext* c)
{
	c->var_mom.reset();
	for (JpContext* l : c->lanes) l->var_mom.reset();
}

int variance_render(JpContext* c, const JpRenderParams* rp, float* film_dev, float* var_dev, bool sync)
{
	if (rp->spp < 2) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_variance: spp must be >= 2 (the sample variance of one sample is undefined)");
	c->var_on = true; c->var_dev = var_dev;
	const int st = render_impl(c, rp, film_dev, false);
	c->var_on = false; c->var_dev = nullptr;
	for (JpContext* l : c->lanes) { l->var_on = false; l->var_dev = nullptr; }
	if (st != JP_OK) { release_moments(c); return st; }
	c->last_mom_bytes = (long long)c->var_mom.bytes();
	for (JpContext* l : c->lanes) c->last_mom_bytes += (long long)l->var_mom.bytes();
	if (sync) { HIP_TRY(hipStreamSynchronize(c->stream)); release_moments(c); }
	return JP_OK;
}

int ensure_variance_events(JpContext* c)
{
	for (hipEvent_t* e : { &c->dv_ev[0], &c->dv_ev[1] }) if (!*e) HIP_TRY(hipEventCreate(e));
	return JP_OK;
}

// jp_denoise's checks (under this entry point's name), then the two new buffers: the variance is an input, variance_out an output that may be null
int denoise_v_check(JpContext* c, const JpDenoiseParams* dp, const void* film, const void* albedo, const void* normal, const void* dist, const void* variance, const void* out, const void* var_out, DenoiseSetup& s)
{
	if (const int e = denoise_check(c, dp, film, albedo, normal, dist, out, s); e != JP_OK)
	{
		if (g_err.compare(0, 11, "jp_denoise:") == 0) g_err = "jp_denoise_variance:" + g_err.substr(11);
		return e;
	}
	if (!variance) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise_variance: null buffer");
	if (dp->sigma_color == 0.f) s.sc = JP_DENOISE_V_SIGMA_COLOR;
	const size_t n = (size_t)s.width * s.height * sizeof(float);
	if (overlaps(out, 3 * n, variance, n)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise_variance: out overlaps an input");
	if (var_out)
	{
		const struct { const void* p; size_t bytes; } in[5] = { { film, 3 * n }, { albedo, 3 * n }, { normal, 3 * n }, { dist, n }, { variance, n } };
		for (const auto& i : in) if (overlaps(var_out, n, i.p, i.bytes)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise_variance: variance_out overlaps an input");
		if (overlaps(var_out, n, out, 3 * n)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_denoise_variance: variance_out overlaps out");
	}
	return JP_OK;
}

int denoise_v_launch(JpContext* c, const DenoiseSetup& s, const float* film, const float* albedo, const float* normal, const float* dist, const float* variance, float* out, float* var_out)
{
	HIP_TRY(hipSetDevice(c->device));
	if (const int e = ensure_variance_events(c); e != JP_OK) return e;
	const size_t npix = (size_t)s.width * s.height;
	for (DevBuf* b : { &c->dn_cz[0], &c->dn_cz[1], &c->dn_nr, &c->dn_nv })      // the records: colours and normals + variance, both ping-pong: 64 bytes per pixel
		if (const int e = reserve_idle(c, *b, npix * 16); e != JP_OK) return e;
	float4* const cz[2] = { c->dn_cz[0].get<float4>(), c->dn_cz[1].get<float4>() }; float4* const nv[2] = { c->dn_nr.get<float4>(), c->dn_nv.get<float4>() };
	const float* alb = s.demod ? albedo : nullptr;
	AtrousVConst ac = { s.width, s.height, 1, s.sc * s.sc, 1.0f / (s.sn * s.sn), 1.0f / (s.sz * s.sz), (c->film_on && c->film_state.hdr) ? 1 : 0 };
	HIP_TRY(hipEventRecord(c->dv_ev[0], c->stream));
	hipLaunchKernelGGL(k_atrous_v_pack, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream,
	                   (int)npix, film, alb, normal, dist, variance, cz[0], nv[0]);
	const dim3 grid((s.width + JP_ATROUS_TW - 1) / JP_ATROUS_TW, (s.height + JP_ATROUS_TH - 1) / JP_ATROUS_TH);
	for (int i = 0; i < s.iterations; i++)
	{
		ac.step = 1 << i;
		const int a = i & 1, b = a ^ 1;
		if (i + 1 < s.iterations) hipLaunchKernelGGL(k_atrous_v<false>, grid, dim3(JP_BLOCK), 0, c->stream, ac, (const float4*)cz[a], (const float4*)nv[a], cz[b], nv[b], (const float*)nullptr, (float*)nullptr, (float*)nullptr);
		else hipLaunchKernelGGL(k_atrous_v<true>, grid, dim3(JP_BLOCK), 0, c->stream, ac, (const float4*)cz[a], (const float4*)nv[a], (float4*)nullptr, (float4*)nullptr, alb, out, var_out);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->dv_ev[1], c->stream));
	c->dv_timed = true; c->last_dv = s.iterations; c->last_dv_sigma[0] = s.sc; c->last_dv_sigma[1] = s.sn; c->last_dv_sigma[2] = s.sz; c->last_dv_demod = s.demod ? 1 : 0;
	return JP_OK;
}
}

extern "C" {

int jp_variance_samples(const JpFilm* f, int32_t spp, int64_t n_pixels, const float* samples_rgb, float* variance_out, float* mean_out)
{
	if (spp < 2) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_samples: spp must be >= 2 (the sample variance of one sample is undefined)");
	if (n_pixels < 0 || (n_pixels > 0 && (!samples_rgb || (!variance_out && !mean_out)))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_samples: null argument");
	if (f) if (const int e = film_check_status(f); e != JP_OK) return e;
	jp_var_samples(f ? f->sample_clamp : 0.f, spp, n_pixels, samples_rgb, variance_out, mean_out);
	return JP_OK;
}

int jp_variance_probe(JpContext* c, const JpFilm* f, int32_t spp, int32_t batch_spp, int64_t n_pixels, const float* samples_rgb, float* variance_out)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_probe: null context");
	if (spp < 2) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_probe: spp must be >= 2 (the sample variance of one sample is undefined)");
	if (batch_spp < 1) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_probe: batch_spp must be >= 1");
	if (n_pixels < 0 || n_pixels > (1ll << 28) || (long long)spp * n_pixels > (1ll << 30)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_probe: bad n_pixels (at most 2^28 pixels and 2^30 samples)");
	if (n_pixels > 0 && (!samples_rgb || !variance_out)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_variance_probe: null argument");
	if (f) if (const int e = film_check_status(f); e != JP_OK) return e;
	if (n_pixels == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_s, b_m, b_v; float* d_s; float2* d_m; float* d_v;         // per-call scratch: freed on every return
	const size_t ns = (size_t)spp * (size_t)n_pixels * 3;
	HIP_TRY(reserve(b_s, d_s, ns * sizeof(float))); HIP_TRY(reserve(b_m, d_m, (size_t)n_pixels * sizeof(float2))); HIP_TRY(reserve(b_v, d_v, (size_t)n_pixels * sizeof(float)));
	HIP_TRY(hipMemcpyAsync(d_s, samples_rgb, ns * sizeof(float), hipMemcpyHostToDevice, c->stream));
	const unsigned int grid = (unsigned int)std::min<long long>((long long)c->n_cus * 8, (n_pixels + JP_BLOCK - 1) / JP_BLOCK);
	for (int s0 = 0; s0 < spp; s0 += batch_spp)
		hipLaunchKernelGGL(k_var_probe, dim3(grid), dim3(JP_BLOCK), 0, c->stream, (long long)n_pixels, spp, s0, std::min(batch_spp, spp - s0), (const float*)d_s, d_m, d_v, f ? f->sample_clamp : 0.f);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(variance_out, d_v, (size_t)n_pixels * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_render_variance_device(JpContext* c, const JpRenderParams* rp, void* film_dev, void* variance_dev, int sync)
{
	if (!c || !rp || !film_dev || !variance_dev) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_variance: null argument");
	if (rp->width > 0 && rp->height > 0 && overlaps(film_dev, (size_t)rp->width * rp->height * 12, variance_dev, (size_t)rp->width * rp->height * 4)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_variance: the variance plane overlaps the film");
	return variance_render(c, rp, (float*)film_dev, (float*)variance_dev, sync != 0);
}

int jp_render_variance(JpContext* c, const JpRenderParams* rp, float* film_host, float* variance_host)
{
	if (!c || !rp || (!film_host && !variance_host)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_variance: null argument");
	if (rp->width <= 0 || rp->height <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_variance: bad width/height");
	HIP_TRY(hipSetDevice(c->device));
	const size_t npix = (size_t)rp->width * rp->height;
	if (const int e = ensure_film(c, 3 * npix); e != JP_OK) return e;
	if (const int e = reserve_idle(c, c->var_plane, npix * sizeof(float)); e != JP_OK) return e;
	float* const d_film = c->film.get<float>(); float* const d_var = c->var_plane.get<float>();
	if (const int e = variance_render(c, rp, d_film, d_var, false); e != JP_OK) return e;
	if (film_host) HIP_TRY(hipMemcpyAsync(film_host, d_film, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (variance_host) HIP_TRY(hipMemcpyAsync(variance_host, d_var, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	release_moments(c);
	return JP_OK;
}

int jp_denoise_variance_device(JpContext* c, const JpDenoiseParams* dp, const void* film_dev, const void* albedo_dev, const void* normal_dev, const void* depth_dev, const void* variance_dev,
                               void* out_dev, void* variance_out_dev, int sync)
{
	DenoiseSetup s;
	if (const int e = denoise_v_check(c, dp, film_dev, albedo_dev, normal_dev, depth_dev, variance_dev, out_dev, variance_out_dev, s); e != JP_OK) return e;
	if (const int e = denoise_v_launch(c, s, (const float*)film_dev, (const float*)albedo_dev, (const float*)normal_dev, (const float*)depth_dev, (const float*)variance_dev, (float*)out_dev, (float*)variance_out_dev); e != JP_OK) return e;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_denoise_variance(JpContext* c, const JpDenoiseParams* dp, const float* film, const float* albedo, const float* normal, const float* depth, const float* variance, float* out, float* variance_out)
{
	DenoiseSetup s;
	if (const int e = denoise_v_check(c, dp, film, albedo, normal, depth, variance, out, variance_out, s); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)s.width * s.height;
	if (const int e = ensure_stage(c, 15 * n); e != JP_OK) return e;
	float *df = c->dn_stage.get<float>(), *da = df + 3 * n, *dn = df + 6 * n, *dz = df + 9 * n, *dout = df + 10 * n, *dv = df + 13 * n, *dvo = df + 14 * n;
	HIP_TRY(hipMemcpyAsync(df, film, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (s.demod) HIP_TRY(hipMemcpyAsync(da, albedo, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dn, normal, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dz, depth, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(dv, variance, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (const int e = denoise_v_launch(c, s, df, da, dn, dz, dv, dout, variance_out ? dvo : nullptr); e != JP_OK) return e;
	HIP_TRY(hipMemcpyAsync(out, dout, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (variance_out) HIP_TRY(hipMemcpyAsync(variance_out, dvo, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

// jp_render_variance, jp_render_guides, jp_denoise_variance and the tone map of jp_render_rgb8 in one call: everything stays on the device between the stages
int jp_render_denoised_variance(JpContext* c, const JpRenderParams* rp, int32_t guide_spp, const JpDenoiseParams* dp, float* film_host, uint8_t* rgb8_host, float* albedo, float* normal, float* depth, float* variance)
{
	if (!c || !rp || (!film_host && !rgb8_host)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_render_denoised_variance: null argument");
	GuideConst gc;
	if (const int e = guides_check(c, rp, guide_spp, gc); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)gc.width * gc.height;
	if (const int e = ensure_stage(c, 11 * n); e != JP_OK) return e;
	float *da = c->dn_stage.get<float>(), *dn = da + 3 * n, *dz = da + 6 * n, *dout = da + 7 * n, *dv = da + 10 * n;
	if (const int e = ensure_film(c, 3 * n); e != JP_OK) return e;
	float* const film = c->film.get<float>();
	DenoiseSetup s;
	if (dp)
	{
		JpDenoiseParams d = *dp; d.width = gc.width; d.height = gc.height;
		if (const int e = denoise_v_check(c, &d, film, da, dn, dz, dv, dout, nullptr, s); e != JP_OK) return e;
	}
	if (const int e = variance_render(c, rp, film, dv, false); e != JP_OK) return e;
	if (const int e = guides_launch(c, gc, da, dn, dz); e != JP_OK) return e;
	const float* result = film;
	if (dp) { if (const int e = denoise_v_launch(c, s, film, da, dn, dz, dv, dout, nullptr); e != JP_OK) return e; result = dout; }
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
	if (variance) HIP_TRY(hipMemcpyAsync(variance, dv, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	release_moments(c);
	return JP_OK;
}

int jp_get_variance_info(JpContext* c, JpVarianceInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_variance_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_variance_info: set JpVarianceInfo.struct_bytes to sizeof(JpVarianceInfo)");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	JpVarianceInfo i; std::memset(&i, 0, sizeof(i));
	i.variance_last_render = c->last_var; i.moment_bytes_device = c->last_var ? c->last_mom_bytes : 0;
	i.iterations = c->last_dv; i.sigma_color = c->last_dv_sigma[0]; i.sigma_normal = c->last_dv_sigma[1]; i.sigma_depth = c->last_dv_sigma[2]; i.demodulated = c->last_dv_demod;
	float ms = 0.f;
	if (c->dv_timed && hipEventElapsedTime(&ms, c->dv_ev[0], c->dv_ev[1]) == hipSuccess) i.denoise_ms = ms;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

} // extern "C"

#endif // JP_VARIANCE_RUNTIME
