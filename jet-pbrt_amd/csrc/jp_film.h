// jet-pbrt_amd/csrc/jp_film.h -- the film (include/jetpbrt_amd.h "Film", DESIGN.md "Film"): film state (unclamped output, per-sample firefly clamp), the luminance
// histogram and the display transform.  The definitions -- the sample clamp, the histogram bin, the curves, the exposure -- are include/jp_film.h and
// include/jp_tonemap.h, shared with the host.  Two parts, like jp_normals.h: part 1 (the shared text, before the kernels: k_resolve_film next to k_resolve in
// jp_kernels.hip calls it) and, with JP_FILM_RUNTIME defined, part 2 LAST: k_film_hist, k_display and the entry points.  Nothing before part 2 refers to anything
// in it but film_to_rgb8 (declared by jp_render.h) and the context's film state (jp_runtime.h); with no film state and no tone map set none of it runs.
#ifndef JP_FILM_DEVICE_PART
#define JP_FILM_DEVICE_PART
#include "../../include/jp_film.h"
#include "../../include/jp_tonemap.h"
#endif // JP_FILM_DEVICE_PART

#if defined(JP_FILM_RUNTIME) && !defined(JP_FILM_RUNTIME_PART)
#define JP_FILM_RUNTIME_PART

// ---------------------------------------------------------------------------------------------------------------------
// k_film_hist: one read pass over a tightly packed rgb film (12 B per pixel), launched like k_tonemap8.  Per workgroup a histogram of JP_FILM_BINS + 1 counters
// in LDS (LDS atomics; the last counter: the excluded pixels), then one global atomicAdd per non-empty counter.  Integer counts: the order does not matter.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JP_BLOCK) k_film_hist(const float* __restrict__ film, unsigned int* __restrict__ hist, size_t npix)
{
	static_assert(JP_BLOCK == JP_FILM_BINS, "one thread per bin");
	__shared__ unsigned int s_h[JP_FILM_BINS + 1];
	s_h[threadIdx.x] = 0u;
	if (threadIdx.x == 0) s_h[JP_FILM_BINS] = 0u;
	__syncthreads();
	for (size_t p = (size_t)blockIdx.x * JP_BLOCK + threadIdx.x; p < npix; p += (size_t)gridDim.x * JP_BLOCK)
		atomicAdd(&s_h[jp_film_bin(film[3 * p], film[3 * p + 1], film[3 * p + 2])], 1u);
	__syncthreads();
	const unsigned int v = s_h[threadIdx.x];
	if (v) atomicAdd(&hist[threadIdx.x], v);
	if (threadIdx.x == 0 && s_h[JP_FILM_BINS]) atomicAdd(&hist[JP_FILM_BINS], s_h[JP_FILM_BINS]);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_display: jp_tm_value per value of the film, an instance per curve (CLAMP: one multiplication more than k_tonemap8), then the floats and / or the byte --
// k_tonemap8's threshold search in LDS.  Either output may be null; neither may overlap the film.
// ---------------------------------------------------------------------------------------------------------------------
template <int kCurve>
__global__ void __launch_bounds__(JP_BLOCK) k_display(const float* __restrict__ film, unsigned char* __restrict__ rgb8, float* __restrict__ out, const float* __restrict__ thr,
                                                       size_t n, float scale, float w2)
{
	__shared__ float s_thr[256];
	s_thr[threadIdx.x] = threadIdx.x < 255 ? thr[threadIdx.x] : JP_INF;
	__syncthreads();
	for (size_t i = (size_t)blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * JP_BLOCK)
	{
		const float y = jp_tm_value(kCurve, w2, scale, film[i]);
		if (out) out[i] = y;
		if (rgb8) rgb8[i] = (unsigned char)jp_tm_byte(s_thr, y);
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace
{
int film_check_status(const JpFilm* f)
{
	switch (jp_film_check(f))
	{
	case 0: return JP_OK;
	case 1: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_film: set JpFilm.struct_bytes to sizeof(JpFilm)");
	case 2: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_film: hdr must be 0 or 1");
	default: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_film: sample_clamp must be finite and >= 0 (0: off)");
	}
}

int tonemap_check_status(const JpToneMap* t, JpToneMap& resolved)
{
	switch (jp_tonemap_resolve(t, &resolved))
	{
	case 0: return JP_OK;
	case 1: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: set JpToneMap.struct_bytes to sizeof(JpToneMap)");
	case 2: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: unknown curve (JP_CURVE_CLAMP .. JP_CURVE_HABLE)");
	case 3: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: unknown exposure_mode (JP_EXPOSURE_MANUAL, JP_EXPOSURE_AUTO)");
	case 4: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: ev must be finite");
	case 5: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: key must be finite and > 0 (0: the default, 0.18)");
	case 6: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: white must be finite and > 0 (0: the default, 4)");
	default: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: the percentiles must be finite with 0 <= pct_low < pct_high <= 1 (0: the defaults, 0.05 and 0.95)");
	}
}

// the tone map a call runs: the caller's, checked, or the one in force
int tonemap_of(JpContext* c, const JpToneMap* t, JpToneMap& tm)
{
	if (t) return tonemap_check_status(t, tm);
	if (!c->tonemap_on) return fail(JP_ERR_INVALID_ARGUMENT, "jp_tonemap: no tone map given and none in force (jp_set_tonemap)");
	tm = c->tonemap;
	return JP_OK;
}

int film_dims(const char* who, int32_t w, int32_t h)
{
	if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 28)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": bad width/height");
	return JP_OK;
}

int ensure_film_events(JpContext* c)
{
	for (hipEvent_t* e : { &c->fh_ev[0], &c->fh_ev[1], &c->tm_ev[0], &c->tm_ev[1] }) if (!*e) HIP_TRY(hipEventCreate(e));
	return JP_OK;
}

// hist_dev: JP_FILM_BINS + 1 dwords, zeroed on the stream first
int hist_launch(JpContext* c, const float* film_dev, size_t npix, unsigned int* hist_dev)
{
	if (const int e = ensure_film_events(c); e != JP_OK) return e;
	HIP_TRY(hipMemsetAsync(hist_dev, 0, (JP_FILM_BINS + 1) * sizeof(unsigned int), c->stream));
	HIP_TRY(hipEventRecord(c->fh_ev[0], c->stream));
	hipLaunchKernelGGL(k_film_hist, dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (npix + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream, film_dev, hist_dev, npix);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->fh_ev[1], c->stream));
	c->fh_timed = true;
	return JP_OK;
}

// the exposure scale of `tm` for the film at film_dev: AUTO runs the histogram into the context's buffer and reads it back (synchronises the stream)
int exposure_of(JpContext* c, const JpToneMap& tm, const float* film_dev, size_t npix, float& scale)
{
	if (tm.exposure_mode == JP_EXPOSURE_MANUAL) { scale = jp_tonemap_exposure(&tm, nullptr); return JP_OK; }
	if (const int e = reserve_idle(c, c->film_hist, (JP_FILM_BINS + 1) * sizeof(unsigned int)); e != JP_OK) return e;
	if (const int e = hist_launch(c, film_dev, npix, c->film_hist.get<unsigned int>()); e != JP_OK) return e;
	uint32_t h[JP_FILM_BINS + 1];
	HIP_TRY(hipMemcpyAsync(h, c->film_hist.get<void>(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	scale = jp_tonemap_exposure(&tm, h);
	return JP_OK;
}

typedef void (*DisplayKernel)(const float*, unsigned char*, float*, const float*, size_t, float, float);
DisplayKernel display_kernel(int curve)
{
	return curve == JP_CURVE_REINHARD ? k_display<JP_CURVE_REINHARD> : (curve == JP_CURVE_ACES ? k_display<JP_CURVE_ACES> : (curve == JP_CURVE_HABLE ? k_display<JP_CURVE_HABLE> : k_display<JP_CURVE_CLAMP>));
}

// exposure, then k_display: npix pixels at film_dev -> rgb8_dev and / or rgb_dev, on the context's stream
int display_launch(JpContext* c, const JpToneMap& tm, const float* film_dev, size_t npix, unsigned char* rgb8_dev, float* rgb_dev, float* scale_out)
{
	if (const int e = ensure_gamma(c); e != JP_OK) return e;
	if (const int e = ensure_film_events(c); e != JP_OK) return e;
	float scale = 1.f;
	if (const int e = exposure_of(c, tm, film_dev, npix, scale); e != JP_OK) return e;
	const size_t n = 3 * npix;
	HIP_TRY(hipEventRecord(c->tm_ev[0], c->stream));
	hipLaunchKernelGGL(display_kernel(tm.curve), dim3((unsigned int)std::min<size_t>((size_t)c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK)), dim3(JP_BLOCK), 0, c->stream,
	                   film_dev, rgb8_dev, rgb_dev, c->gamma.get<const float>(), n, scale, tm.white * tm.white);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->tm_ev[1], c->stream));
	c->tm_timed = true; c->last_scale = scale;
	if (scale_out) *scale_out = scale;
	return JP_OK;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) { return a && b && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }
}

// jp_render_rgb8 / jp_render_denoised: the film at src -> c->rgb8 (ensure_rgb8 has run)
static int film_to_rgb8(JpContext* c, const float* src, int width, int height)
{
	const size_t npix = (size_t)width * height;
	c->last_tonemapped = 0;
	if (!c->tonemap_on) { tonemap8(c, src, 3 * npix); return JP_OK; }
	if (const int e = display_launch(c, c->tonemap, src, npix, c->rgb8.get<unsigned char>(), nullptr, nullptr); e != JP_OK) return e;
	c->last_tonemapped = 1;
	return JP_OK;
}

extern "C" {

int jp_check_film(const JpFilm* f)
{
	if (!f) return JP_OK;                                              // NULL: the reference's film
	return film_check_status(f);
}

int jp_set_film(JpContext* c, const JpFilm* f)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_film: null context");
	if (f) if (const int e = film_check_status(f); e != JP_OK) return e;
	c->film_state = JpFilm(); c->film_on = false;
	if (f && (f->hdr || f->sample_clamp > 0.f)) { c->film_state = *f; c->film_state.struct_bytes = (int32_t)sizeof(JpFilm); c->film_on = true; }   // read by the next jp_render* / jp_denoise*
	return JP_OK;
}

int jp_get_film_info(JpContext* c, JpFilmInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_film_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_film_info: set JpFilmInfo.struct_bytes to sizeof(JpFilmInfo)");
	JpFilmInfo i; std::memset(&i, 0, sizeof(i));
	if (c->film_on) { i.hdr = c->film_state.hdr; i.sample_clamp = c->film_state.sample_clamp; }
	i.hdr_last_render = c->last_hdr;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_film_samples(const JpFilm* f, int32_t n, const float* in_rgb, float* out_rgb)
{
	if (n < 0 || (n > 0 && (!in_rgb || !out_rgb))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_film_samples: null argument");
	if (f) if (const int e = film_check_status(f); e != JP_OK) return e;
	const float c = f ? f->sample_clamp : 0.f;
	for (int32_t i = 0; i < n; i++)
	{
		float r = in_rgb[3 * (size_t)i], g = in_rgb[3 * (size_t)i + 1], b = in_rgb[3 * (size_t)i + 2];
		if (c > 0.f) jp_film_clamp_sample(c, &r, &g, &b);
		out_rgb[3 * (size_t)i] = r; out_rgb[3 * (size_t)i + 1] = g; out_rgb[3 * (size_t)i + 2] = b;
	}
	return JP_OK;
}

int jp_film_histogram_device(JpContext* c, int32_t width, int32_t height, const void* film_dev, void* hist_dev, int sync)
{
	if (!c || !film_dev || !hist_dev) return fail(JP_ERR_INVALID_ARGUMENT, "jp_film_histogram: null argument");
	if (const int e = film_dims("jp_film_histogram", width, height); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	if (const int e = hist_launch(c, (const float*)film_dev, (size_t)width * height, (unsigned int*)hist_dev); e != JP_OK) return e;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_film_histogram(JpContext* c, int32_t width, int32_t height, const float* film_rgb, uint32_t* hist)
{
	if (!c || !film_rgb || !hist) return fail(JP_ERR_INVALID_ARGUMENT, "jp_film_histogram: null argument");
	if (const int e = film_dims("jp_film_histogram", width, height); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t npix = (size_t)width * height;
	if (const int e = reserve_idle(c, c->film_stage, 3 * npix * sizeof(float)); e != JP_OK) return e;
	if (const int e = reserve_idle(c, c->film_hist, (JP_FILM_BINS + 1) * sizeof(unsigned int)); e != JP_OK) return e;
	HIP_TRY(hipMemcpyAsync(c->film_stage.get<void>(), film_rgb, 3 * npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (const int e = hist_launch(c, c->film_stage.get<const float>(), npix, c->film_hist.get<unsigned int>()); e != JP_OK) return e;
	HIP_TRY(hipMemcpyAsync(hist, c->film_hist.get<void>(), (JP_FILM_BINS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_check_tonemap(const JpToneMap* t)
{
	if (!t) return JP_OK;                                              // NULL: none
	JpToneMap r;
	return tonemap_check_status(t, r);
}

int jp_set_tonemap(JpContext* c, const JpToneMap* t)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_tonemap: null context");
	JpToneMap r = {};
	if (t) if (const int e = tonemap_check_status(t, r); e != JP_OK) return e;
	c->tonemap = r; c->tonemap_on = t != nullptr;                      // read by the next jp_render_rgb8 / jp_render_denoised / jp_tonemap(NULL)
	return JP_OK;
}

int jp_exposure_from_histogram(const JpToneMap* t, const uint32_t* hist, float* scale_out)
{
	if (!t || !scale_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_exposure_from_histogram: null argument");
	JpToneMap r;
	if (const int e = tonemap_check_status(t, r); e != JP_OK) return e;
	if (r.exposure_mode == JP_EXPOSURE_AUTO && !hist) return fail(JP_ERR_INVALID_ARGUMENT, "jp_exposure_from_histogram: JP_EXPOSURE_AUTO needs a histogram");
	*scale_out = jp_tonemap_exposure(&r, hist);
	return JP_OK;
}

int jp_tonemap_host(const JpToneMap* t, float scale, int64_t n_values, const float* in, uint8_t* rgb8_out, float* rgb_out)
{
	if (!t || n_values < 0 || (n_values > 0 && (!in || (!rgb8_out && !rgb_out)))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_tonemap_host: null argument");
	JpToneMap r;
	if (const int e = tonemap_check_status(t, r); e != JP_OK) return e;
	float thr[256];
	std::memcpy(thr, host_gamma_thresholds(), 255 * sizeof(float)); thr[255] = INFINITY;
	const float w2 = r.white * r.white;
	for (int64_t i = 0; i < n_values; i++)
	{
		const float y = jp_tm_value(r.curve, w2, scale, in[i]);
		if (rgb_out) rgb_out[i] = y;
		if (rgb8_out) rgb8_out[i] = (uint8_t)jp_tm_byte(thr, y);
	}
	return JP_OK;
}

int jp_tonemap_device(JpContext* c, const JpToneMap* t, int32_t width, int32_t height, const void* film_dev, void* rgb8_dev, void* rgb_dev, float* scale_out, int sync)
{
	if (!c || !film_dev || (!rgb8_dev && !rgb_dev)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_tonemap: null argument");
	if (const int e = film_dims("jp_tonemap", width, height); e != JP_OK) return e;
	JpToneMap tm;
	if (const int e = tonemap_of(c, t, tm); e != JP_OK) return e;
	const size_t npix = (size_t)width * height;
	if (overlaps(film_dev, 12 * npix, rgb_dev, 12 * npix) || overlaps(film_dev, 12 * npix, rgb8_dev, 3 * npix)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_tonemap: an output overlaps the film");
	HIP_TRY(hipSetDevice(c->device));
	if (const int e = display_launch(c, tm, (const float*)film_dev, npix, (unsigned char*)rgb8_dev, (float*)rgb_dev, scale_out); e != JP_OK) return e;
	if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_tonemap(JpContext* c, const JpToneMap* t, int32_t width, int32_t height, const float* film_rgb, uint8_t* rgb8_out, float* rgb_out, float* scale_out)
{
	if (!c || !film_rgb || (!rgb8_out && !rgb_out)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_tonemap: null argument");
	if (const int e = film_dims("jp_tonemap", width, height); e != JP_OK) return e;
	JpToneMap tm;
	if (const int e = tonemap_of(c, t, tm); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	const size_t npix = (size_t)width * height, n = 3 * npix;
	// staging: the film, the floats, the bytes (n + n floats, then n bytes)
	if (const int e = reserve_idle(c, c->film_stage, 2 * n * sizeof(float) + n); e != JP_OK) return e;
	float* const d_film = c->film_stage.get<float>(); float* const d_out = d_film + n; unsigned char* const d_rgb8 = (unsigned char*)(d_out + n);
	HIP_TRY(hipMemcpyAsync(d_film, film_rgb, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	if (const int e = display_launch(c, tm, d_film, npix, rgb8_out ? d_rgb8 : nullptr, rgb_out ? d_out : nullptr, scale_out); e != JP_OK) return e;
	if (rgb8_out) HIP_TRY(hipMemcpyAsync(rgb8_out, d_rgb8, n, hipMemcpyDeviceToHost, c->stream));
	if (rgb_out) HIP_TRY(hipMemcpyAsync(rgb_out, d_out, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_get_tonemap_info(JpContext* c, JpToneMapInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_tonemap_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_tonemap_info: set JpToneMapInfo.struct_bytes to sizeof(JpToneMapInfo)");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	JpToneMapInfo i; std::memset(&i, 0, sizeof(i));
	if (c->tonemap_on) { i.curve = c->tonemap.curve; i.exposure_mode = c->tonemap.exposure_mode; }
	i.scale_last = c->last_scale; i.mapped_last_render = c->last_tonemapped;
	float ms = 0.f;
	if (c->fh_timed && hipEventElapsedTime(&ms, c->fh_ev[0], c->fh_ev[1]) == hipSuccess) i.histogram_ms = ms;
	if (c->tm_timed && hipEventElapsedTime(&ms, c->tm_ev[0], c->tm_ev[1]) == hipSuccess) i.tonemap_ms = ms;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

} // extern "C"

#endif // JP_FILM_RUNTIME
