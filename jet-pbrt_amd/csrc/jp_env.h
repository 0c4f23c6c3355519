// jet-pbrt_amd/csrc/jp_env.h -- environment maps (INTEGRATION.md "Environment maps", DESIGN.md "Environment maps"): a lat-long fp32 image as the one
// environment light of a JP_LIGHTS_POWER_ONE scene, looked up by nearest texel on a miss and importance-sampled by texel for next-event estimation.
// Two parts, because shade_body needs the device functions and the runtime needs the context:
//   part 1 (included by jp_kernels.hip before the kernels): EnvView, env_lookup, env_sample;
//   part 2 (JP_ENV_RUNTIME, included after jp_pick.h): k_shade_env / k_shade_env_tex (shade_body<..., kPick, kEnv>), the test hook k_env_probe, the upload's
//   table step and the entry points jp_set_environment_map / jp_get_env_info / jp_env_lookup / jp_env_sample / jp_build_environment_table.
// The kernels are selected and launched with every other k_shade family (shade_choice, jp_render.h; shade_launch, jp_shade_launch.h).
// A context that never binds a map runs nothing of this file.
#ifndef JP_ENV_DEVICE_PART
#define JP_ENV_DEVICE_PART
// ---- part 1: the view and the two device functions -------------------------------------------------------------------------------
// A separate kernel argument like TexView / PickView: SceneView, Queues, RenderConst, PickView and TexView stay as they are.
struct EnvView
{
	const float4* texel;         // per texel, row-major, top row first: tinted (r, g, b), pdf_t = (float)((w_t / W_env) / Omega_r)
	const float2* bins;          // alias table over the W * H texels: (threshold q, alias as int bits)
	const float2* rows;          // per row: ((float)cos(pi r / H), (float)cos(pi (r + 1) / H))
	int W, H, up, light;         // size, JP_ENV_UP_*, index of the map light in the scene's light list
	float row_scale, col_scale;  // (float)H / pi, (float)W / (2 pi): direction -> texel coordinate
	float phi_step;              // 2 pi / (float)W
};
// world space -> map space and back: JP_ENV_UP_Z is the identity, JP_ENV_UP_Y map (x, y, z) = world (z, x, y)
__device__ __forceinline__ V3 env_to_map(const EnvView& ev, V3 d) { return ev.up == JP_ENV_UP_Y ? mk(d.z, d.x, d.y) : d; }
__device__ __forceinline__ V3 env_to_world(const EnvView& ev, V3 m) { return ev.up == JP_ENV_UP_Y ? mk(m.y, m.z, m.x) : m; }

// the texel a world-space direction sees (nearest texel: the sampler's density is exactly proportional to what this returns)
__device__ __forceinline__ int env_lookup(const EnvView& ev, V3 d)
{
	const V3 m = env_to_map(ev, d);
	const float theta = acosf(clampf(m.z, -1.f, 1.f));
	float phi = atan2f(m.y, m.x); if (phi < 0.f) phi += JP_2PI;
	int row = (int)(theta * ev.row_scale), col = (int)(phi * ev.col_scale);
	row = row < ev.H - 1 ? row : ev.H - 1; col = col < ev.W - 1 ? col : ev.W - 1;
	row = row > 0 ? row : 0; col = col > 0 ? col : 0;                 // (a direction that is not a number must not index below the table)
	return row * ev.W + col;
}

// one next-event sample of the map from the five draws a0 a1 a2 (the texel, through the alias table) b0 b1 (the place inside it): texel index, world-space wi,
// Li and pdf straight from the texel record (taken, not looked up again)
__device__ __forceinline__ int env_sample(const EnvView& ev, float a0, float a1, float a2, float b0, float b1, V3& wi, V3& Li, float& pdf)
{
	int r0 = (int)(a0 * (float)ev.H), c0 = (int)(a1 * (float)ev.W);
	r0 = r0 < ev.H - 1 ? r0 : ev.H - 1; c0 = c0 < ev.W - 1 ? c0 : ev.W - 1;
	const int i = r0 * ev.W + c0;
	const float2 b = ev.bins[i];
	const int j = a2 < b.x ? i : __float_as_int(b.y);
	const int r = j / ev.W, c = j - r * ev.W;
	const float4 t = ev.texel[j];
	const float2 rcs = ev.rows[r];
	const float dc = rcs.x - rcs.y, cosT = rcs.x - b1 * dc;
	// sin^2 = (1 - cos)(1 + cos) with the factor that is small taken from the row's edge, where it is exact at a pole (ct = 1, cb = -1): 1 - cos^2 itself
	// rounds to 0 within 3.5e-4 rad of a pole, an error of up to 1e-4 in wi (b1 = 1 - 2^-24 in the last row)
	const float omc = (1 - rcs.x) + b1 * dc, opc = (1 + rcs.y) + (1 - b1) * dc;
	const float sinT = sqrtf(smax(0.f, cosT >= 0.f ? omc * (2 - omc) : opc * (2 - opc)));
	const float phi = ((float)c + b0) * ev.phi_step;
	float sinP, cosP; sincos_f(phi, &sinP, &cosP);
	wi = env_to_world(ev, mk(sinT * cosP, sinT * sinP, cosT));
	Li = xyz(t); pdf = t.w;
	return j;
}
#endif // JP_ENV_DEVICE_PART

#if defined(JP_ENV_RUNTIME) && !defined(JP_ENV_RUNTIME_PART)
#define JP_ENV_RUNTIME_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------
// k_shade_pick with the map as the scene's one environment light: a miss adds the texel the ray sees, and when the alias table of the lights
// returns the map light the sample comes from env_sample (five draws in place of the light's two)
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_env(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, EnvView ev)
{
	const TexView tv = {}; const MisView mv = {};
	shade_body<kTab, kPrims, kStage, kSort, false, true, true, false>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
template <bool kTab, bool kPrims, bool kStage, bool kSort>
__global__ void __launch_bounds__(JP_BLOCK) k_shade_env_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, EnvView ev)
{
	const MisView mv = {};
	shade_body<kTab, kPrims, kStage, kSort, true, true, true, false>(sc, q, rc, cur, cnt, tv, pv, ev, mv);
}
// jp_env_lookup (mode 0: in = 3 floats a direction) / jp_env_sample (mode 1: in = 5 floats a sample): the functions the render calls
__global__ void __launch_bounds__(JP_BLOCK) k_env_probe(EnvView ev, int mode, int n, const float* __restrict__ in, int* __restrict__ index, float* __restrict__ wi, float* __restrict__ Li, float* __restrict__ pdf)
{
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		if (mode == 0)
		{
			const int j = env_lookup(ev, mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
			const float4 t = ev.texel[j];
			index[i] = j; Li[3 * i] = t.x; Li[3 * i + 1] = t.y; Li[3 * i + 2] = t.z;
		}
		else
		{
			V3 w, L; float p;
			const int j = env_sample(ev, in[5 * i], in[5 * i + 1], in[5 * i + 2], in[5 * i + 3], in[5 * i + 4], w, L, p);
			index[i] = j; wi[3 * i] = w.x; wi[3 * i + 1] = w.y; wi[3 * i + 2] = w.z; Li[3 * i] = L.x; Li[3 * i + 1] = L.y; Li[3 * i + 2] = L.z; pdf[i] = p;
		}
	}
}

// the upload's map step (jp_upload_scene with a map bound, before upload_light_table): the refusals, the tables (build_environment_table, jp_scene_host.h),
// their device copies into the upload's tables T and the plan's ev; mean_sum is what upload_light_table weighs the map light with
static int upload_environment_map(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, bool pick)
{
	const EnvMapHost& m = c->env_map;
	if (!pick) return fail(JP_ERR_UNSUPPORTED, "jp_upload_scene: an environment map needs JP_LIGHTS_POWER_ONE (jp_set_light_sampling); the map light is one entry of the light table");
	int n_env = 0, at = -1;
	for (int i = 0; i < s->n_lights; i++) if (s->light_type[i] == JP_LIGHT_ENVIRONMENT) { n_env++; at = i; }
	if (n_env == 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: an environment map is bound but the scene has no JP_LIGHT_ENVIRONMENT light (its light_radiance is the map's tint)");
	if (n_env > 1) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: an environment map is bound and the scene has more than one JP_LIGHT_ENVIRONMENT light");
	JpEnvMap map; map.struct_bytes = (int32_t)sizeof(JpEnvMap); map.width = m.W; map.height = m.H; map.up_axis = m.up; map.importance = m.importance; map.rgb = m.rgb.data();
	EnvTables e;
	if (const int st = build_environment_table(&map, s->light_radiance + 3 * (size_t)at, e); st != JP_OK) return st;
	const size_t n = (size_t)m.W * m.H;
	std::vector<float2> bins(n);
	for (size_t i = 0; i < n; i++) { float af; std::memcpy(&af, &e.alias[i], 4); bins[i] = make_float2(e.q[i], af); }
	HIP_TRY(upload(T.env_texel, e.texel.data(), n * sizeof(float4)));
	HIP_TRY(upload(T.env_bins, bins.data(), n * sizeof(float2)));
	HIP_TRY(upload(T.env_rows, e.row_cos.data(), (size_t)m.H * sizeof(float2)));
	EnvView& ev = plan.ev; ev = EnvView();
	ev.texel = T.env_texel.get<float4>(); ev.bins = T.env_bins.get<float2>(); ev.rows = T.env_rows.get<float2>();
	ev.W = m.W; ev.H = m.H; ev.up = m.up; ev.light = at;
	ev.row_scale = (float)m.H / JP_PI; ev.col_scale = (float)m.W / JP_2PI; ev.phi_step = JP_2PI / (float)m.W;
	plan.env = true; plan.env_mean_sum = e.mean_sum;
	c->env_n_selectable = e.n_selectable; c->env_total_weight = e.total; c->env_table_bytes = (long long)(T.env_texel.bytes() + T.env_bins.bytes() + T.env_rows.bytes());
	return JP_OK;
}

extern "C" {

int jp_build_environment_table(const JpEnvMap* map, const float* tint, double* weight, float* q, int32_t* alias, float* texel, float* row_cos, double* total, double* mean_sum)
{
	if (!map) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_environment_table: null map");
	const float one[3] = { 1.f, 1.f, 1.f };
	EnvTables e;
	if (const int st = build_environment_table(map, tint ? tint : one, e); st != JP_OK) return st;
	const size_t n = (size_t)map->width * map->height;
	if (weight) std::memcpy(weight, e.weight.data(), n * sizeof(double));
	if (q) std::memcpy(q, e.q.data(), n * sizeof(float));
	if (alias) std::memcpy(alias, e.alias.data(), n * sizeof(int32_t));
	if (texel) std::memcpy(texel, e.texel.data(), n * sizeof(float4));
	if (row_cos) std::memcpy(row_cos, e.row_cos.data(), (size_t)map->height * sizeof(float2));
	if (total) *total = e.total;
	if (mean_sum) *mean_sum = e.mean_sum;
	return JP_OK;
}

int jp_set_environment_map(JpContext* c, const JpEnvMap* map)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_environment_map: null context");
	if (!map) { c->env_map = EnvMapHost(); return JP_OK; }               // read by the next jp_upload_scene*
	if (const int st = check_environment_map("jp_set_environment_map", map); st != JP_OK) return st;
	EnvMapHost m; m.W = map->width; m.H = map->height; m.up = map->up_axis; m.importance = map->importance;
	m.rgb.assign(map->rgb, map->rgb + 3 * (size_t)m.W * m.H);
	c->env_map = std::move(m);
	return JP_OK;
}

int jp_get_env_info(JpContext* c, JpEnvInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_env_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_env_info: set JpEnvInfo.struct_bytes to sizeof(JpEnvInfo)");
	JpEnvInfo i; std::memset(&i, 0, sizeof(i));
	const bool on = c->plan.have_scene && c->plan.env;                   // the uploaded scene's map (all 0 without one)
	if (on)
	{
		i.width = c->plan.ev.W; i.height = c->plan.ev.H; i.up_axis = c->plan.ev.up; i.importance = c->env_importance;
		i.n_selectable = c->env_n_selectable; i.total_weight = c->env_total_weight; i.mean_sum = c->plan.env_mean_sum; i.table_bytes_device = c->env_table_bytes;
	}
	i.mapped_last_render = c->last_mapped;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

// both probes: n records of `per` floats in, the kernel, the results out (any result pointer may be NULL)
static int env_probe(JpContext* c, const char* who, int mode, int32_t n, const float* in, int per, int32_t* index, float* wi, float* Li, float* pdf)
{
	if (!c || n < 0 || !in) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, std::string(who) + ": no scene uploaded");
	if (!c->plan.env) return fail(JP_ERR_UNSUPPORTED, std::string(who) + ": the scene was uploaded without an environment map");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_in, b_i, b_o; float *d_in, *d_o; int* d_i;                 // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * per * 4)); HIP_TRY(reserve(b_i, d_i, (size_t)n * 4)); HIP_TRY(reserve(b_o, d_o, (size_t)n * 7 * 4));
	float *d_wi = d_o, *d_Li = d_o + 3 * (size_t)n, *d_pdf = d_o + 6 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_in, in, (size_t)n * per * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(k_env_probe, dim3(grid), dim3(JP_BLOCK), 0, c->stream, c->plan.ev, mode, n, (const float*)d_in, d_i, d_wi, d_Li, d_pdf);
	HIP_TRY(hipGetLastError());
	if (index) HIP_TRY(hipMemcpyAsync(index, d_i, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	if (wi && mode == 1) HIP_TRY(hipMemcpyAsync(wi, d_wi, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	if (Li) HIP_TRY(hipMemcpyAsync(Li, d_Li, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	if (pdf && mode == 1) HIP_TRY(hipMemcpyAsync(pdf, d_pdf, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

int jp_env_lookup(JpContext* c, int32_t n, const float* dir, int32_t* texel_index, float* rgb)
{
	if (dir && n > 0) for (size_t i = 0; i < 3 * (size_t)n; i++) if (!std::isfinite(dir[i])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_env_lookup: a direction is not finite");
	return env_probe(c, "jp_env_lookup", 0, n, dir, 3, texel_index, nullptr, rgb, nullptr);
}

int jp_env_sample(JpContext* c, int32_t n, const float* u, int32_t* texel_index, float* wi, float* Li, float* pdf)
{
	if (u && n > 0) for (size_t i = 0; i < 5 * (size_t)n; i++) if (!(u[i] >= 0.f && u[i] < 1.f)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_env_sample: a draw outside [0, 1)");   // (what the samplers deliver; the bin index is not clamped from below)
	return env_probe(c, "jp_env_sample", 1, n, u, 5, texel_index, wi, Li, pdf);
}

} // extern "C"
#endif // JP_ENV_RUNTIME
