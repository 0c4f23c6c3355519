// jet-pbrt_amd/csrc/jp_pick.h -- light selection (JP_LIGHTS_POWER_ONE; INTEGRATION.md "Light selection", DESIGN.md "Light selection"): the alias table
// builder's entry point (the builder itself: build_light_table, jp_scene_host.h), the upload's table step, k_shade_pick / k_shade_pick_tex (shade_body<..., kPick>), the test hook k_light_pick and the entry points
// jp_set_light_sampling / jp_get_light_info / jp_get_light_table / jp_light_pick / jp_build_light_table.  Included last by jp_kernels.hip: a context that
// never switches the mode on runs nothing of this file.  The kernels are selected and launched with every other k_shade family (shade_choice, jp_render.h; shade_launch, jp_shade_launch.h).
#pragma once

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// k_shade with ONE next-event light per bounce: the light from the alias table (light_pick, jp_common.h), its records from global memory
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_pick(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv)
{
	const TexView tv = {}; const EnvView ev = {}; const MisView mv = {};
	shade_body<kTab, kPrims, kStage, kSort, false, true, false, false>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_pick_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv)
{
	const EnvView ev = {}; const MisView mv = {};
	shade_body<kTab, kPrims, kStage, kSort, true, true, false, false>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
// jp_light_pick: the render's selection for n pairs of draws
__global__ void __launch_bounds__(JP_BLOCK) k_light_pick(PickView pv, int n, const float* __restrict__ u0, const float* __restrict__ u1, int* __restrict__ index, float* __restrict__ pmf)
{
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		float pm = 0.f; int j = -1;
		if (pv.n > 0) j = light_pick(pv, u0[i], u1[i], pm);
		index[i] = j; pmf[i] = pm;
	}
}

// the upload's table step (jp_upload_scene, mode JP_LIGHTS_POWER_ONE): weights, table, the environment list, the device copies into the upload's
// tables T, and its plan's pv
static int upload_light_table(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const std::vector<float>& area)
{
	const int n = s->n_lights;
	const double kPi = 3.14159265358979323846;
	std::vector<double> w((size_t)n); std::vector<float4> env;
	for (int i = 0; i < n; i++)
	{
		const float* rad = s->light_radiance + 3 * (size_t)i;
		const double sum = ((double)rad[0] + (double)rad[1]) + (double)rad[2];
		const int ty = s->light_type[i];
		if (ty == JP_LIGHT_AREA) w[i] = (sum * (double)area[i]) * kPi;
		else if (ty == JP_LIGHT_POINT) w[i] = sum * (4.0 * kPi);
		else if (plan.env && ty == JP_LIGHT_ENVIRONMENT) w[i] = (plan.env_mean_sum * kPi) * ((double)s->world_radius * (double)s->world_radius);   // the map light (jp_env.h): the map's mean in place of the sum
		else w[i] = (sum * kPi) * ((double)s->world_radius * (double)s->world_radius);          // light.cc:17-33
		if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: a light's power is negative or not finite (JP_LIGHTS_POWER_ONE)");
		if (ty == JP_LIGHT_ENVIRONMENT && !(rad[0] == 0.f && rad[1] == 0.f && rad[2] == 0.f)) { float lf; const int32_t li = i; std::memcpy(&lf, &li, 4); env.push_back(make_float4(rad[0], rad[1], rad[2], lf)); }   // (.w: the light's index as int bits, for jp_mis.h)
	}
	std::vector<float> q((size_t)std::max(1, n), 0.f), pmf((size_t)std::max(1, n), 0.f); std::vector<int32_t> alias((size_t)std::max(1, n), 0);
	double W = 0.0; int nsel = 0;
	if (const int st = build_light_table(n, w.data(), q.data(), alias.data(), pmf.data(), &W, &nsel); st != JP_OK) return st;
	std::vector<float2> bins((size_t)std::max(1, n), make_float2(0.f, 0.f));
	for (int i = 0; i < n; i++) { float af; std::memcpy(&af, &alias[i], 4); bins[i] = make_float2(q[i], af); }
	const int n_env = (int)env.size();
	if (env.empty()) env.push_back(make_float4(0, 0, 0, 0));         // (never read: n_env is 0)
	HIP_TRY(upload(T.pick_bins, bins.data(), bins.size() * sizeof(float2)));
	HIP_TRY(upload(T.pick_pmf, pmf.data(), pmf.size() * sizeof(float)));
	HIP_TRY(upload(T.pick_env, env.data(), env.size() * sizeof(float4)));
	PickView& pv = plan.pv;
	pv.bins = T.pick_bins.get<float2>(); pv.pmf = T.pick_pmf.get<float>(); pv.env = T.pick_env.get<float4>(); pv.n = n; pv.n_env = n_env;
	plan.pick = true; c->n_selectable = nsel; c->total_weight = W;
	return JP_OK;
}

extern "C" {

int jp_build_light_table(int32_t n, const double* weight, float* q, int32_t* alias, float* pmf)
{
	if (n < 0 || (n > 0 && !weight)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_light_table: bad count or null weights");
	return build_light_table(n, weight, q, alias, pmf, nullptr, nullptr);
}

int jp_set_light_sampling(JpContext* c, const JpLightSampling* ls)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_light_sampling: null context");
	int mode = JP_LIGHTS_ALL;
	if (ls)
	{
		if (ls->struct_bytes < (int32_t)sizeof(JpLightSampling)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_light_sampling: set JpLightSampling.struct_bytes to sizeof(JpLightSampling)");
		if (ls->mode != JP_LIGHTS_ALL && ls->mode != JP_LIGHTS_POWER_ONE) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_light_sampling: unknown mode");
		mode = ls->mode;
	}
	c->light_mode = mode;                                              // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_light_info(JpContext* c, JpLightInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_light_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_light_info: set JpLightInfo.struct_bytes to sizeof(JpLightInfo)");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_get_light_info: no scene uploaded");
	JpLightInfo i; std::memset(&i, 0, sizeof(i));
	i.mode = c->plan.pick ? JP_LIGHTS_POWER_ONE : JP_LIGHTS_ALL; i.n_lights = c->plan.sv.n_lights;
	i.n_selectable = c->plan.pick ? c->n_selectable : (c->plan.sv.n_lights > 0 ? c->plan.n_planes : 0);
	i.total_weight = c->plan.pick ? c->total_weight : 0.0; i.picked_last_render = c->last_picked;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_get_light_table(JpContext* c, float* q, int32_t* alias, float* pmf)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_light_table: null context");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_get_light_table: no scene uploaded");
	if (!c->plan.pick) return fail(JP_ERR_UNSUPPORTED, "jp_get_light_table: the scene was uploaded with JP_LIGHTS_ALL (no table)");
	const int n = c->plan.pv.n;
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	std::vector<float2> bins((size_t)n);
	HIP_TRY(hipMemcpy(bins.data(), c->plan.pv.bins, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost));
	for (int i = 0; i < n; i++) { if (q) q[i] = bins[i].x; if (alias) std::memcpy(&alias[i], &bins[i].y, 4); }
	if (pmf) HIP_TRY(hipMemcpy(pmf, c->plan.pv.pmf, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
	return JP_OK;
}

int jp_light_pick(JpContext* c, int32_t n, const float* u0, const float* u1, int32_t* index, float* pmf)
{
	if (!c || n < 0 || !u0 || !u1 || !index || !pmf) return fail(JP_ERR_INVALID_ARGUMENT, "jp_light_pick: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_light_pick: no scene uploaded");
	if (!c->plan.pick) return fail(JP_ERR_UNSUPPORTED, "jp_light_pick: the scene was uploaded with JP_LIGHTS_ALL (no table)");
	if (n == 0) return JP_OK;
	for (int i = 0; i < n; i++) if (!(u0[i] >= 0.f && u0[i] < 1.f) || !(u1[i] >= 0.f && u1[i] < 1.f)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_light_pick: a draw outside [0, 1)");   // (what the samplers deliver; the bin index is not clamped from below)
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_u, b_i, b_p; float *d_u, *d_p; int* d_i;                // per-call scratch: freed on every return
	HIP_TRY(reserve(b_u, d_u, (size_t)n * 8)); HIP_TRY(reserve(b_i, d_i, (size_t)n * 4)); HIP_TRY(reserve(b_p, d_p, (size_t)n * 4));
	HIP_TRY(hipMemcpyAsync(d_u, u0, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_u + n, u1, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(k_light_pick, dim3(grid), dim3(JP_BLOCK), 0, c->stream, c->plan.pv, n, (const float*)d_u, (const float*)(d_u + n), d_i, d_p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(index, d_i, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(pmf, d_p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

} // extern "C"
