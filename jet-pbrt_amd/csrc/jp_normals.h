// jet-pbrt_amd/csrc/jp_normals.h -- interpolated shading normals (INTEGRATION.md "Vertex normals", DESIGN.md "Smooth normals"), in two parts like jp_env.h:
//   part 1 (included before the kernels): NormView and shading_normal, the device side of include/jp_normals.h
//   part 2 (JP_NORMALS_RUNTIME, included after jp_render.h and jp_denoise.h): k_normal, the smooth twins of the ten k_shade families (shade_body<..., kSmooth>), the test
//     hook k_shading_normal, the upload's table step and the entry points jp_set_vertex_normals / jp_get_normal_info / jp_shading_normal / jp_interpolate_normals.
// k_normal is launched by launch_normal, the smooth twins by shade_launch with every other k_shade family (jp_shade_launch.h, included after this part).
// A context that never sets vertex normals runs nothing of this file.
#ifndef JP_NORMALS_DEVICE_PART
#define JP_NORMALS_DEVICE_PART
#include "jp_common.h"
#include "../../include/jp_normals.h"

// ---- part 1 -----------------------------------------------------------------------------------------------------------------------------
// A separate kernel argument like TexView: SceneView, Queues and RenderConst stay as they are, so the kernels of scenes without normals do not change.
struct NormView
{
	const float4* prim_vn;       // three per primitive of the caller's order: (n0, smooth flag) (n1, -) (n2, -); 48 contiguous bytes, all 0 for flat triangles and other shapes
	float4* side;                // one record per queue position: (Ns, 1) where the ray hit a smooth triangle, else 0 (k_normal -> k_shade_smooth*)
};

namespace jp
{
// Ns at the point p of device primitive h (caller's primitive index = meta.x); false: not a smooth triangle (Ns untouched)
__device__ __forceinline__ bool shading_normal(const float4* prims, const NormView& nv, int h, int prim, V3 p, V3& Ns)
{
	const float4 g3 = prims[4 * h + 3];
	if (__float_as_int(g3.w) != JP_SHAPE_TRIANGLE) return false;
	const float4 v0 = nv.prim_vn[3 * prim], v1 = nv.prim_vn[3 * prim + 1], v2 = nv.prim_vn[3 * prim + 2];
	if (v0.w == 0.f) return false;
	const float4 g0 = prims[4 * h], g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
	const float a0[3] = { g0.x, g0.y, g0.z }, a1[3] = { g1.x, g1.y, g1.z }, a2[3] = { g2.x, g2.y, g2.z }, ng[3] = { g3.x, g3.y, g3.z }, ap[3] = { p.x, p.y, p.z };
	const float vn9[9] = { v0.x, v0.y, v0.z, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z };
	float ns[3];
	jp_shading_normal_at(a0, a1, a2, ng, vn9, ap, ns);
	Ns = mk(ns[0], ns[1], ns[2]);
	return true;
}
} // namespace jp
#endif // JP_NORMALS_DEVICE_PART

#if defined(JP_NORMALS_RUNTIME) && !defined(JP_NORMALS_RUNTIME_PART)
#define JP_NORMALS_RUNTIME_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------------
// k_normal: for every queued ray of the block's region that hit a smooth triangle, Ns of the hit as one 16-byte side record at the ray's queue position
// (w = 0: not smooth).  Kept out of k_shade like k_texel, and for the same reason: the dependent gather hit -> primitive record -> caller's index -> nine
// normals hides behind 8 waves per SIMD here, and k_shade's registers (3 waves) stay out of it.
__global__ void __launch_bounds__(JP_BLOCK, 8) k_normal(SceneView sc, Queues q, int cur, NormView nv)
{
	const unsigned int b = blockIdx.x, n = q.blk_q[cur][b], rbase = b * q.R;
	for (unsigned int j = threadIdx.x; j < n; j += JP_BLOCK)
	{
		const unsigned int i = rbase + j;
		const float2 h = q.hit[i];
		const int pi = __float_as_int(h.y);
		float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
		if (pi >= 0)
		{
			const float4 ro = q.ray_o[cur][i], rd = q.ray_d[cur][i];
			const V3 p = xyz(ro) + h.x * xyz(rd);                                   // ray(distance), as k_shade forms it
			V3 Ns;
			if (shading_normal(sc.prims, nv, pi, sc.meta[pi].x, p, Ns)) rec = make_float4(Ns.x, Ns.y, Ns.z, 1.f);
		}
		nv.side[i] = rec;
	}
}

// The smooth twins of the ten families.  One row each: the tables in global memory (<false, false, false>, the row a large mesh takes anyway) x sort; the upload
// plans a smooth scene onto that row (upload_vertex_normals).
#define JP_SMOOTH_BODY(kSort, kTex, kPick, kEnv, kMis) shade_body<false, false, false, kSort, kTex, kPick, kEnv, kMis, FeatAll, false, true>(sc, q, rc, cur, cnt, tv, pv, ev, mv, nv)
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, NormView nv)
{ const TexView tv = {}; const PickView pv = {}; const EnvView ev = {}; const MisView mv = {}; JP_SMOOTH_BODY(kSort, false, false, false, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, NormView nv)
{ const PickView pv = {}; const EnvView ev = {}; const MisView mv = {}; JP_SMOOTH_BODY(kSort, true, false, false, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_pick(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, NormView nv)
{ const TexView tv = {}; const EnvView ev = {}; const MisView mv = {}; JP_SMOOTH_BODY(kSort, false, true, false, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_pick_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, NormView nv)
{ const EnvView ev = {}; const MisView mv = {}; JP_SMOOTH_BODY(kSort, true, true, false, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_env(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, EnvView ev, NormView nv)
{ const TexView tv = {}; const MisView mv = {}; JP_SMOOTH_BODY(kSort, false, true, true, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_env_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, EnvView ev, NormView nv)
{ const MisView mv = {}; JP_SMOOTH_BODY(kSort, true, true, true, false); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_mis(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, MisView mv, NormView nv)
{ const TexView tv = {}; const EnvView ev = {}; JP_SMOOTH_BODY(kSort, false, true, false, true); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_mis_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, MisView mv, NormView nv)
{ const EnvView ev = {}; JP_SMOOTH_BODY(kSort, true, true, false, true); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_mis_env(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, PickView pv, EnvView ev, MisView mv, NormView nv)
{ const TexView tv = {}; JP_SMOOTH_BODY(kSort, false, true, true, true); }
template <bool kSort> __global__ void __launch_bounds__(JP_BLOCK, 3) k_shade_smooth_mis_env_tex(SceneView sc, Queues q, RenderConst rc, int cur, DevCounters* cnt, TexView tv, PickView pv, EnvView ev, MisView mv, NormView nv)
{ JP_SMOOTH_BODY(kSort, true, true, true, true); }
#undef JP_SMOOTH_BODY

// k_shading_normal (jp_shading_normal): the closest hit of k_trace's walk, Ng as k_trace returns it and the Ns the render uses there
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_shading_normal(SceneView sc, NormView nv, int smooth, int depth, int n, const float* o, const float* d, const float* tmin, const float* tmax_in,
                                                                int* prim, float* ng, float* ns)
{
	SceneAccess<kMode> acc(sc, depth);
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
		float tmax = tmax_in[i];
		const int h = acc.template trace<false>(sc, ro, rd, tmin[i], tmax);
		V3 N = mk(0, 0, 0), Ns = N; int pr = -1;
		if (h >= 0)
		{
			const float4 g3 = sc.prims[4 * h + 3]; const int type = __float_as_int(g3.w);
			const V3 p = ro + tmax * rd;
			pr = sc.meta[h].x;
			if (type == JP_SHAPE_TRIANGLE) N = xyz(g3);
			else if (type == JP_SHAPE_RECTANGLE) N = dot(xyz(g3), rd) <= 0 ? xyz(g3) : -xyz(g3);
			else if (type == JP_SHAPE_DISK) N = xyz(sc.prims[4 * h + 1]);
			else N = normalize(p - xyz(sc.prims[4 * h]));
			Ns = N;
			if (smooth) shading_normal(sc.prims, nv, h, pr, p, Ns);
		}
		prim[i] = pr;
		ng[3 * i] = N.x; ng[3 * i + 1] = N.y; ng[3 * i + 2] = N.z;
		ns[3 * i] = Ns.x; ns[3 * i + 1] = Ns.y; ns[3 * i + 2] = Ns.z;
	}
}

namespace
{
typedef void (*ShadingNormalKernel)(SceneView, NormView, int, int, int, const float*, const float*, const float*, const float*, int*, float*, float*);
// the instance that belongs to the k_trace trace_kernel selects
ShadingNormalKernel shading_normal_kernel(const TraceLaunch& t) { return by_trace_mode(t.mode, [](auto m) -> ShadingNormalKernel { return k_shading_normal<decltype(m)::value>; }); }

// nine values per triangle as the ABI takes them; which: the first offending triangle
int check_vertex_normals(int n, const float* vn, int& n_smooth)
{
	n_smooth = 0;
	for (int i = 0; i < n; i++)
	{
		const int k = jp_vertex_normals_class(vn + 9 * (size_t)i);
		if (k < 0)
		{
			bool finite = true; for (int j = 0; j < 9; j++) if (!std::isfinite(vn[9 * (size_t)i + j])) finite = false;
			return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: triangle " + std::to_string(i) + (finite ? ": a normal's squared length is outside [0.81, 1.21] (nine zeros mark a flat triangle)" : ": a value is not finite"));
		}
		n_smooth += k;
	}
	return JP_OK;
}
}

// the upload's table step (jp_upload_scene with vertex normals set): the 48-byte records in the caller's primitive order, and the plan of a smooth scene --
// k_shade's row <false, false, false> (tables in global memory, no staging), which is where the smooth instances exist
static int upload_vertex_normals(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s)
{
	const VertexNormalsHost& v = c->vnormals;
	if (v.n_triangles != s->n_triangles) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the vertex normals' n_triangles differs from the scene's (jp_set_vertex_normals)");
	c->vn_triangles = v.n_triangles; c->vn_smooth = v.n_smooth; c->vn_table_bytes = 0;
	if (v.n_smooth == 0) return JP_OK;                                  // all flat: the scene without normals, exactly
	std::vector<float4> rec(3 * (size_t)std::max(1, s->n_primitives), make_float4(0.f, 0.f, 0.f, 0.f));
	for (int p = 0; p < s->n_primitives; p++)
	{
		if (s->prim_shape_type[p] != JP_SHAPE_TRIANGLE) continue;
		const float* n9 = v.vn.data() + 9 * (size_t)s->prim_shape_index[p];
		if (jp_vertex_normals_class(n9) != 1) continue;
		for (int k = 0; k < 3; k++) rec[3 * (size_t)p + k] = make_float4(n9[3 * k], n9[3 * k + 1], n9[3 * k + 2], k == 0 ? 1.f : 0.f);
	}
	HIP_TRY(upload(T.prim_vn, rec.data(), rec.size() * sizeof(float4)));
	plan.nv = NormView(); plan.nv.prim_vn = T.prim_vn.get<float4>();
	plan.smooth = true;
	plan.tables_in_lds = false; plan.shade_prims_in_lds = false; plan.stage_nee = false; plan.shade_lds_bytes = 0;
	c->vn_table_bytes = (long long)(rec.size() * sizeof(float4));
	return JP_OK;
}

// the side records of a context's queue set (render_one of a smooth scene: cap positions)
static int ensure_normal_side(JpContext* c, unsigned int cap, NormView& nv)
{
	if (const int e = reserve_idle(c, c->nside, (size_t)cap * sizeof(float4)); e != JP_OK) return e;
	nv.side = c->nside.get<float4>();
	return JP_OK;
}

extern "C" {

int jp_set_vertex_normals(JpContext* c, const JpVertexNormals* vn)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: null context");
	if (!vn) { c->vnormals = VertexNormalsHost(); return JP_OK; }
	if (vn->struct_bytes < (int32_t)sizeof(JpVertexNormals)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: set JpVertexNormals.struct_bytes to sizeof(JpVertexNormals)");
	if (vn->n_triangles < 0 || (vn->n_triangles > 0 && !vn->tri_vn)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: bad n_triangles or null tri_vn");
	int ns = 0;
	if (const int st = check_vertex_normals(vn->n_triangles, vn->tri_vn, ns); st != JP_OK) return st;
	VertexNormalsHost h; h.set = true; h.n_triangles = vn->n_triangles; h.n_smooth = ns;
	h.vn.assign(vn->tri_vn, vn->tri_vn + 9 * (size_t)vn->n_triangles);
	c->vnormals = std::move(h);                                        // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_normal_info(JpContext* c, JpNormalInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_normal_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_normal_info: set JpNormalInfo.struct_bytes to sizeof(JpNormalInfo)");
	JpNormalInfo i; std::memset(&i, 0, sizeof(i));
	if (c->plan.have_scene) { i.n_triangles = c->vn_triangles; i.n_smooth_triangles = c->vn_smooth; i.table_bytes_device = c->vn_table_bytes; }
	i.smooth_last_render = c->last_smooth;
	if (c->profiling && c->last_smooth)
	{   // k_normal's launches of the last render, all lanes (HIP-event times; synchronises)
		if (const int st = finish_counters(c); st != JP_OK) return st;
		i.normal_ms = c->normal_ms; for (int k = 1; k < c->last_lanes; k++) i.normal_ms += c->lanes[k - 1]->normal_ms;
	}
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_interpolate_normals(int32_t n, const float* p0, const float* p1, const float* p2, const float* ng, const float* vn9, const float* p, float* ns_out)
{
	if (n < 0 || (n > 0 && (!p0 || !p1 || !p2 || !ng || !vn9 || !p || !ns_out))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_interpolate_normals: null argument");
	for (int32_t i = 0; i < n; i++) jp_shading_normal_at(p0 + 3 * (size_t)i, p1 + 3 * (size_t)i, p2 + 3 * (size_t)i, ng + 3 * (size_t)i, vn9 + 9 * (size_t)i, p + 3 * (size_t)i, ns_out + 3 * (size_t)i);
	return JP_OK;
}

int jp_check_vertex_normals(const JpVertexNormals* vn, int32_t* n_smooth)
{
	if (!vn) return fail(JP_ERR_INVALID_ARGUMENT, "jp_check_vertex_normals: null argument");
	if (vn->struct_bytes < (int32_t)sizeof(JpVertexNormals)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: set JpVertexNormals.struct_bytes to sizeof(JpVertexNormals)");
	if (vn->n_triangles < 0 || (vn->n_triangles > 0 && !vn->tri_vn)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_vertex_normals: bad n_triangles or null tri_vn");
	int ns = 0;
	const int st = check_vertex_normals(vn->n_triangles, vn->tri_vn, ns);
	if (st == JP_OK && n_smooth) *n_smooth = ns;
	return st;
}

int jp_shading_normal(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, int32_t* prim, float* ng, float* ns)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !prim || !ng || !ns) return fail(JP_ERR_INVALID_ARGUMENT, "jp_shading_normal: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_shading_normal: no scene uploaded");
	if (n == 0) return JP_OK;
	const TraceLaunch tk = trace_kernel(c->plan, c->opt.trace_walk, true);      // the walk jp_trace takes (generic: the instance with every shape's normal)
	const ShadingNormalKernel k = shading_normal_kernel(tk);
	const ShadingNormalMappedKernel km = c->plan.mapped ? shading_normal_mapped_kernel(tk) : nullptr;   // normal maps (jp_normal_map.h): the hook's twin
	if (!k || (c->plan.mapped && !km)) return fail(JP_ERR_UNSUPPORTED, "jp_shading_normal: no instance for this scene's walk");
	HIP_TRY(hipSetDevice(c->device));
	DevBuf b_in, b_g, b_s, b_prim; float *d_in, *d_g, *d_s; int* d_prim;        // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 32)); HIP_TRY(reserve(b_g, d_g, (size_t)n * 12)); HIP_TRY(reserve(b_s, d_s, (size_t)n * 12)); HIP_TRY(reserve(b_prim, d_prim, (size_t)n * 4));
	float *d_o = d_in, *d_d = d_in + 3 * (size_t)n, *d_t0 = d_in + 6 * (size_t)n, *d_t1 = d_in + 7 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	if (km) hipLaunchKernelGGL(km, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.nv, c->plan.mp, c->plan.sm, tk.depth, n, (const float*)d_o, (const float*)d_d, (const float*)d_t0, (const float*)d_t1, d_prim, d_g, d_s);
	else hipLaunchKernelGGL(k, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.nv, c->plan.smooth ? 1 : 0, tk.depth, n, (const float*)d_o, (const float*)d_d, (const float*)d_t0, (const float*)d_t1, d_prim, d_g, d_s);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(prim, d_prim, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(ng, d_g, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(ns, d_s, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

} // extern "C"
#endif // JP_NORMALS_RUNTIME
