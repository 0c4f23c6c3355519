// jet-pbrt_amd/csrc/jp_lens_runtime.h -- thin-lens camera (include/jetpbrt_amd.h "Lens", DESIGN.md "Lens"): the test hook k_camera_rays and the entry points.
// The definition itself -- JpLensPlan, the lens sample, the ray -- is include/jp_lens.h, shared with the host; k_raygen<true>, k_other and k_guides call it through
// camera_ray (jp_kernels.hip).  Included by jp_kernels.hip LAST: the lens state of the context (jp_runtime.h) is all that the code before it reads.
#pragma once

// k_camera_rays (jp_camera_rays): k_raygen's key, film position and camera_ray for n (pixel, sample) triples
__global__ void __launch_bounds__(JP_BLOCK) k_camera_rays(JpCamera cam, unsigned int seed, int sampler_debug, int lens_on, JpLensPlan lp, JpProjectionPlan pp, int n,
                                                          const int* __restrict__ px, const int* __restrict__ py, const int* __restrict__ ps,
                                                          float* __restrict__ origin, float* __restrict__ dir, int* __restrict__ dim_next)
{
	RenderConst rc; rc.sampler_debug = sampler_debug;                  // (rngf reads nothing else)
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const int x = px[i], y = py[i], s = ps[i];
		const uint32_t key = jp_rng_key(seed, (uint32_t)x, (uint32_t)y, (uint32_t)s);
		const float fx = (float)x + rngf(rc, key, 0), fy = (float)y + rngf(rc, key, 1);
		V3 o, d;
		if (lens_on) camera_ray<true>(cam, &lp, fx, fy, rngf(rc, key, 2), rngf(rc, key, 3), o, d);
		else if (pp.kind != JP_PROJ_PERSPECTIVE) projected_ray(cam, pp, fx, fy, o, d);   // (jp_set_projection: never together with a lens)
		else camera_ray<false>(cam, nullptr, fx, fy, 0.f, 0.f, o, d);
		if (origin) { origin[3 * i] = o.x; origin[3 * i + 1] = o.y; origin[3 * i + 2] = o.z; }
		if (dir) { dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z; }
		if (dim_next) dim_next[i] = lens_on ? 4 : 2;
	}
}

namespace
{
int lens_check_status(const JpLens* l)
{
	switch (jp_lens_check(l))
	{
	case 0: return JP_OK;
	case 1: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: set JpLens.struct_bytes to sizeof(JpLens)");
	case 2: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: radius must be finite and >= 0");
	case 3: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: focus_distance must be finite and > 0 when radius > 0");
	case 4: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: blades must be 0 (a disk) or 3 .. 16");
	default: return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: rotation_deg must be finite");
	}
}
}

extern "C" {

int jp_check_lens(const JpLens* l)
{
	if (!l) return JP_OK;                                              // NULL: the pinhole
	return lens_check_status(l);
}

int jp_set_lens(JpContext* c, const JpLens* l)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_lens: null context");
	if (l) if (const int e = lens_check_status(l); e != JP_OK) return e;
	c->lens = JpLens(); c->lens_on = false;
	if (l && l->radius > 0.f) { c->lens = *l; c->lens.struct_bytes = (int32_t)sizeof(JpLens); c->lens_on = true; }   // read by the next jp_render* / jp_render_guides*
	return JP_OK;
}

int jp_get_lens_info(JpContext* c, JpLensInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_lens_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_lens_info: set JpLensInfo.struct_bytes to sizeof(JpLensInfo)");
	JpLensInfo i; std::memset(&i, 0, sizeof(i));
	if (c->lens_on) { i.radius = c->lens.radius; i.focus_distance = c->lens.focus_distance; i.blades = c->lens.blades; i.rotation_deg = c->lens.rotation_deg; }
	i.lens_last_render = c->last_lens;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_lens_plan(const JpCamera* cam, const JpLens* l, void* plan_out, int64_t capacity, int64_t* bytes)
{
	if (!cam || !bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_plan: null argument");
	*bytes = 0;
	if (l) if (const int e = lens_check_status(l); e != JP_OK) return e;
	if (!l || !(l->radius > 0.f)) return JP_OK;
	JpLensPlan p;
	if (jp_lens_make_plan(cam, l, &p) != 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_plan: the camera's right / up vectors have no finite positive length");
	*bytes = (int64_t)sizeof(p);
	if (!plan_out) return JP_OK;
	if (capacity < (int64_t)sizeof(p)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_plan: capacity smaller than the plan");
	std::memcpy(plan_out, &p, sizeof(p));
	return JP_OK;
}

int jp_lens_rays(const JpCamera* cam, const JpLens* l, int32_t n, const float* fxfy, const float* u, float* origin, float* dir)
{
	if (!cam || n < 0 || !fxfy || !origin || !dir) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_rays: null argument");
	if (l) if (const int e = lens_check_status(l); e != JP_OK) return e;
	const bool on = l && l->radius > 0.f;
	JpLensPlan p;
	if (on)
	{
		if (!u) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_rays: null argument");
		if (jp_lens_make_plan(cam, l, &p) != 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_lens_rays: the camera's right / up vectors have no finite positive length");
	}
	for (int32_t i = 0; i < n; i++)
	{
		if (on) jp_lens_ray(cam, &p, fxfy[2 * i], fxfy[2 * i + 1], u[2 * i], u[2 * i + 1], origin + 3 * (size_t)i, dir + 3 * (size_t)i);
		else jp_pinhole_ray(cam, fxfy[2 * i], fxfy[2 * i + 1], origin + 3 * (size_t)i, dir + 3 * (size_t)i);
	}
	return JP_OK;
}

int jp_camera_rays(JpContext* c, const JpRenderParams* rp, int32_t n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin, float* dir, int32_t* dim_next)
{
	if (!c || !rp || n < 0 || !x || !y || !s) return fail(JP_ERR_INVALID_ARGUMENT, "jp_camera_rays: null argument");
	if (rp->width <= 0 || rp->height <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_camera_rays: bad width/height");
	if (rp->sampler_mode != JP_SAMPLER_COUNTER && rp->sampler_mode != JP_SAMPLER_DEBUG) return fail(JP_ERR_UNSUPPORTED, "jp_camera_rays: the device path implements the counter sampler only (the sequential mt19937_64 stream is not reproducible in parallel)");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_camera_rays: no scene uploaded");
	for (int32_t i = 0; i < n; i++)
		if (x[i] < 0 || x[i] >= rp->width || y[i] < 0 || y[i] >= rp->height || s[i] < 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_camera_rays: pixel or sample index out of range");
	if (n == 0) return JP_OK;
	JpLensPlan lp;
	if (const int e = lens_plan_of(c, lp); e != JP_OK) return e;
	JpProjectionPlan pp;
	if (const int e = proj_plan_of(c, pp); e != JP_OK) return e;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_in, b_o, b_d, b_k; int *d_in, *d_k; float *d_o, *d_d;        // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 12)); HIP_TRY(reserve(b_o, d_o, (size_t)n * 12)); HIP_TRY(reserve(b_d, d_d, (size_t)n * 12)); HIP_TRY(reserve(b_k, d_k, (size_t)n * 4));
	int *d_x = d_in, *d_y = d_in + (size_t)n, *d_s = d_in + 2 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_y, y, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_s, s, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(JP_BLOCK), 0, c->stream, c->plan.sv.cam, (unsigned int)rp->seed, rp->sampler_mode == JP_SAMPLER_DEBUG ? 1 : 0, c->lens_on ? 1 : 0, lp, pp, (int)n,
	                   (const int*)d_x, (const int*)d_y, (const int*)d_s, d_o, d_d, d_k);
	HIP_TRY(hipGetLastError());
	if (origin) HIP_TRY(hipMemcpyAsync(origin, d_o, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	if (dir) HIP_TRY(hipMemcpyAsync(dir, d_d, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	if (dim_next) HIP_TRY(hipMemcpyAsync(dim_next, d_k, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_focus_distance(JpContext* c, float fx, float fy, float* focus_out)
{
	if (!c || !focus_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_focus_distance: null argument");
	*focus_out = 0.f;
	if (!(fx - fx == 0.f) || !(fy - fy == 0.f)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_focus_distance: the film position must be finite");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_focus_distance: no scene uploaded");
	const JpCamera& cam = c->plan.sv.cam;
	float o[3], d[3], d0[3]; jp_pinhole_ray(&cam, fx, fy, o, d); jp_lens_d0(&cam, fx, fy, d0);
	const float tmin = 0.001f, tmax = INFINITY;
	int32_t hit = 0, prim = -1; float t = 0.f, nrm[3];
	if (const int e = jp_trace(c, 1, o, d, &tmin, &tmax, &hit, &t, &prim, nrm); e != JP_OK) return e;
	if (hit) *focus_out = t / jp_lens_length(d0);
	return JP_OK;
}

} // extern "C"
