// jet-pbrt_amd/csrc/jp_mis.h -- multiple importance sampling (JP_ESTIMATOR_MIS; INTEGRATION.md "Estimator", DESIGN.md "Estimator"): the path integrator's two ways
// of reaching an emitter from a non-delta shading event -- a direction drawn on the picked light (next-event estimation) and the direction the BSDF sample
// takes anyway -- weighted against each other with the power heuristic instead of counting the first alone.  Same draws, same rays, other weights.
// Two parts, like jp_env.h:
//   part 1 (included by jp_kernels.hip before the kernels): MisView, mis_weight, pdf_local, light_weighed, light_pdf;
//   part 2 (JP_MIS_RUNTIME, included last): k_shade_mis / _tex / _env / _env_tex (shade_body<..., kPick, kEnv, kMis>), the test hook k_light_pdf and the
//   entry points jp_set_estimator / jp_get_estimator_info / jp_light_pdf.
// The kernels are selected and launched with every other k_shade family (shade_choice, jp_render.h; shade_launch, jp_shade_launch.h).
// A context that never switches the estimator on runs nothing of this file.
#ifndef JP_MIS_DEVICE_PART
#define JP_MIS_DEVICE_PART
// ---- part 1: the view and the device functions ------------------------------------------------------------------------------------
// A separate kernel argument like TexView / PickView / EnvView.  One record per queue position of each of the two ray queues, written by the lane that
// writes ray_o / ray_d / beta there: (pdf the BSDF sample that produced the ray was drawn with, distance travelled since that shading point -- not 0 only
// behind null-material primitives, which pass a path on without a shading event)
struct MisView { float2* side[2]; };

// power heuristic, exponent 2, for the strategy with pdf `own` against the one with pdf `other`: own^2 / (own^2 + other^2) as 1 / (1 + (other / own)^2), which
// cannot turn two large finite pdfs into inf / inf; other == 0 gives exactly 1
__device__ __forceinline__ float mis_weight(float own, float other) { const float r = other / own; return 1.f / (1.f + r * r); }

// the pdf sample_local reports for the direction wi of the chosen closure (local frame; closure_set_wo done): Lambert bsdf.h:362-377, microfacet bsdf.cc:60-78
__device__ __forceinline__ float pdf_local(const Closure& c, V3 wo, V3 wi)
{
	if (!same_hemi(wo, wi)) return 0.f;
	if (c.kind == CL_LAMBERT) return fabsf(wi.z) * JP_INV_PI;
	if (c.kind != CL_MICROFACET) return 0.f;                          // delta closures: no density
	V3 wh = wi + wo;
	if (wh.x == 0 && wh.y == 0 && wh.z == 0) return 0.f;
	wh = normalize(wh);
	return tr_Pdf(c, wo, wh) / (4 * dot(wo, wh));
}

// Does light li take part in the weighting when sampled from p?  Delta lights (point, direction) do not: no BSDF sample reaches them.  A sphere light whose
// interior holds p does not either: sample_li's pdf there depends on the shading normal (shape.h:567-586), so that case stays with next-event estimation.
template <typename PrimPtr, typename LightPtr>
__device__ __forceinline__ bool light_weighed(PrimPtr prims, LightPtr lights, int li, V3 p)
{
	const int lt = __float_as_int(lights[2 * li].w);
	if (lt == JP_LIGHT_ENVIRONMENT) return true;
	if (lt != JP_LIGHT_AREA) return false;
	const int pi = __float_as_int(lights[2 * li + 1].x);
	if (__float_as_int(prims[4 * pi + 3].w) != JP_SHAPE_SPHERE) return true;
	const float4 g0 = prims[4 * pi];
	return !(len2(p - xyz(g0)) <= g0.w * g0.w);
}

// The light strategy's pdf, with respect to solid angle at p, of "the ray from p along d reached light li" (after dist, at a point with normal N_hit; a miss
// for the environment lights): pmf_li times the value sample_li / env_sample assign to that light and direction.  0: the light cannot be sampled there (a
// product that is not finite or not positive; a delta light).  unweighed: p lies inside the sphere light (light_weighed).  has_map: the scene has a map (ev).
template <typename PrimPtr, typename LightPtr>
__device__ __forceinline__ float light_pdf(const SceneView& sc, PrimPtr prims, LightPtr lights, const PickView& pv, const EnvView& ev, bool has_map, int li, V3 p, V3 d, float dist, V3 N_hit, bool& unweighed)
{
	unweighed = false;
	float pdf;
	if (has_map && li == ev.light) pdf = ev.texel[env_lookup(ev, d)].w;
	else
	{
		const float4 l0 = lights[2 * li], l1 = lights[2 * li + 1];
		const int lt = __float_as_int(l0.w);
		if (lt == JP_LIGHT_ENVIRONMENT)
		{   // light.h:265-291: uniform in (theta, phi) about the world's z axis
			const float sinT = sqrtf(d.x * d.x + d.y * d.y);
			pdf = 1 / (2 * JP_PI * JP_PI * sinT);
		}
		else if (lt != JP_LIGHT_AREA) return 0.f;
		else
		{
			const int pi = __float_as_int(l1.x);
			const float inv_area = l1.y;
			const float4 g0 = prims[4 * pi], g3 = prims[4 * pi + 3];
			const int type = __float_as_int(g3.w);
			if (type != JP_SHAPE_SPHERE)
			{   // FShape::SampleDirection shape.h:124-145
				const V3 ln = type == JP_SHAPE_DISK ? xyz(prims[4 * pi + 1]) : xyz(g3);
				pdf = inv_area * ((dist * dist) / absdot(ln, -d));
			}
			else
			{
				const V3 c = xyz(g0); const float r = g0.w;
				if (len2(p - c) <= r * r) { unweighed = true; return 0.f; }
				const float sin_max = r * (1 / len(p - c));            // shape.h:603-643
				const float cos_max = sqrtf(smax(0.f, 1 - sin_max * sin_max));
				pdf = 1 / (2 * JP_PI * (1 - cos_max));
			}
		}
	}
	const float a = pv.pmf[li] * pdf;
	return (a > 0.f && !isinf(a)) ? a : 0.f;                           // (a NaN fails a > 0)
}
#endif // JP_MIS_DEVICE_PART

#if defined(JP_MIS_RUNTIME) && !defined(JP_MIS_RUNTIME_PART)
#define JP_MIS_RUNTIME_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------
// the pick / map kernels with both strategies weighted: one family per (map, textures), the rows and sort variants of k_shade_pick
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_mis(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, MisView mv)
{
	const TexView tv = {}; const EnvView ev = {};
	shade_body<kTab, kPrims, kStage, kSort, false, true, false, true>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_mis_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, MisView mv)
{
	const EnvView ev = {};
	shade_body<kTab, kPrims, kStage, kSort, true, true, false, true>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_mis_env(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, EnvView ev, MisView mv)
{
	const TexView tv = {};
	shade_body<kTab, kPrims, kStage, kSort, false, true, true, true>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_mis_env_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, EnvView ev, MisView mv)
{
	shade_body<kTab, kPrims, kStage, kSort, true, true, true, true>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}

// jp_light_pdf: n rays through k_trace's walk -> the light reached (the emitter that faces the origin; on a miss the map light, else the first non-black
// constant environment light; -1: nothing emits toward the origin) and the light strategy's pdf for it (light_pdf; 0 where it cannot be sampled)
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_light_pdf(SceneView sc, PickView pv, EnvView ev, int has_map, int depth, int n, const float* o, const float* d, const float* tmin, const float* tmax_in,
                                                        int* light, float* pdf)
{
	SceneAccess<kMode> acc(sc, depth);
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
		float tmax = tmax_in[i];
		const int h = acc.template trace<false>(sc, ro, rd, tmin[i], tmax);
		int li = -1; V3 N = mk(0, 0, 1);
		if (h >= 0)
		{
			const int l = sc.meta[h].z;
			if (l >= 0)
			{
				const float4 g3 = sc.prims[4 * h + 3]; const int type = __float_as_int(g3.w);
				const V3 p = ro + tmax * rd;
				if (type == JP_SHAPE_TRIANGLE) N = xyz(g3);
				else if (type == JP_SHAPE_RECTANGLE) N = dot(xyz(g3), rd) <= 0 ? xyz(g3) : -xyz(g3);
				else if (type == JP_SHAPE_DISK) N = xyz(sc.prims[4 * h + 1]);
				else N = normalize(p - xyz(sc.prims[4 * h]));
				if (dot(N, -rd) > 0.f && !isblack(xyz(sc.lights[2 * l]))) li = l;   // FAreaLight::L light.h:234-238
			}
		}
		else if (has_map) li = ev.light;
		else if (pv.n_env > 0) li = __float_as_int(pv.env[0].w);
		float a = 0.f;
		if (li >= 0) { bool unweighed; a = light_pdf(sc, sc.prims, sc.lights, pv, ev, has_map != 0, li, ro, rd, tmax, N, unweighed); }
		light[i] = li; pdf[i] = a;
	}
}

namespace
{
// k_light_pdf for the walk jp_trace takes by default: the instance that belongs to the k_trace trace_kernel selects
typedef void (*LightPdfKernel)(SceneView, PickView, EnvView, int, int, int, const float*, const float*, const float*, const float*, int*, float*);
LightPdfKernel light_pdf_kernel(const TraceLaunch& t) { return by_trace_mode(t.mode, [](auto m) -> LightPdfKernel { return k_light_pdf<decltype(m)::value>; }); }
}

// the side records of a context's queue set (render_one, first MIS render: cap positions per queue)
static int ensure_mis_side(JpContext* c, unsigned int cap, MisView& mv)
{
	for (int b = 0; b < 2; b++)
	{
		if (const int e = reserve_idle(c, c->mis_side[b], (size_t)cap * sizeof(float2)); e != JP_OK) return e;
		mv.side[b] = c->mis_side[b].get<float2>();
	}
	return JP_OK;
}

extern "C" {

int jp_set_estimator(JpContext* c, const JpEstimator* e)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_estimator: null context");
	int mode = JP_ESTIMATOR_NEE;
	if (e)
	{
		if (e->struct_bytes < (int32_t)sizeof(JpEstimator)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_estimator: set JpEstimator.struct_bytes to sizeof(JpEstimator)");
		if (e->mode != JP_ESTIMATOR_NEE && e->mode != JP_ESTIMATOR_MIS) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_estimator: unknown mode");
		mode = e->mode;
	}
	c->estimator = mode;                                               // read by the next jp_render*
	return JP_OK;
}

int jp_get_estimator_info(JpContext* c, JpEstimatorInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_estimator_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_estimator_info: set JpEstimatorInfo.struct_bytes to sizeof(JpEstimatorInfo)");
	JpEstimatorInfo i; std::memset(&i, 0, sizeof(i));
	i.mode = c->estimator; i.mis_last_render = c->last_mis;
	i.side_bytes_device = (int64_t)(c->mis_side[0].bytes() + c->mis_side[1].bytes());
	for (const JpContext* l : c->lanes) i.side_bytes_device += (int64_t)(l->mis_side[0].bytes() + l->mis_side[1].bytes());
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_light_pdf(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* light, float* pdf)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !light || !pdf) return fail(JP_ERR_INVALID_ARGUMENT, "jp_light_pdf: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_light_pdf: no scene uploaded");
	if (!c->plan.pick) return fail(JP_ERR_UNSUPPORTED, "jp_light_pdf: the scene was uploaded with JP_LIGHTS_ALL (no table)");
	if (n == 0) return JP_OK;
	const TraceLaunch tk = trace_kernel(c->plan, 0);
	const LightPdfKernel k = light_pdf_kernel(tk);
	if (!k) return fail(JP_ERR_UNSUPPORTED, "jp_light_pdf: no instance for this scene's walk");
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_in, b_l, b_p; float *d_in, *d_p; int* d_l;               // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 32)); HIP_TRY(reserve(b_l, d_l, (size_t)n * 4)); HIP_TRY(reserve(b_p, d_p, (size_t)n * 4));
	float *d_o = d_in, *d_d = d_in + 3 * (size_t)n, *d_t0 = d_in + 6 * (size_t)n, *d_t1 = d_in + 7 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(k, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.pv, c->plan.ev, c->plan.env ? 1 : 0, tk.depth, n, (const float*)d_o, (const float*)d_d, (const float*)d_t0, (const float*)d_t1, d_l, d_p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(light, d_l, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(pdf, d_p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

} // extern "C"
#endif // JP_MIS_RUNTIME
