// jet-pbrt_amd/csrc/jp_procedural.h -- procedural textures (INTEGRATION.md "Procedural textures", DESIGN.md "Procedural textures"), in three parts like jp_mipmap.h:
//   part 1 (after jp_mipmap.h's parts 1 and 2): ProcView and proc_sample / proc_hit, the device side of include/jp_procedural.h
//   part 2 (JP_PROCEDURAL_KERNELS, right after part 1): k_texel_p (k_texel_m's twin for a scene with at least one procedural record), k_surface_p (k_surface's) and the test hook k_proc_probe
//   part 3 (JP_PROCEDURAL_RUNTIME, at the end): the upload's steps and the entry points jp_set_texture_procedurals / jp_check_texture_procedurals /
//     jp_get_procedural_info / jp_procedural_lookup / jp_procedural_probe.
// A procedural record changes what the side kernel WRITES, never the word's layout: k_shade_tex* read the same word -- the colour's RGB8 under the image tag, or
// the plain checker's colour index.  The ray cone is jp_mipmap.h's: the second consumer of the two floats per path slot.  A context without a record runs nothing
// of this file.
#ifndef JP_PROCEDURAL_DEVICE_PART
#define JP_PROCEDURAL_DEVICE_PART
#include "jp_common.h"
#include "jp_tex.h"
#include "jp_tex_sampling.h"
#include "jp_mipmap.h"
#define JP_PROC_SINCOSF_DEVICE jp::sincos_f
#include "../../include/jp_procedural.h"

// ---- part 1 -----------------------------------------------------------------------------------------------------------------------------
// A separate kernel argument of k_texel_p, k_proc_probe and the guides only: TexView, SampView, MipView and Queues stay as they are.
struct ProcView
{
	const JpProcDev* rec;        // the records of the textures that have one
	const int* tex;              // per texture of TexView::desc: its record in rec, -1: none; null: the scene has no procedural record
};

namespace jp
{
// the side word of procedural texture t (record k) at the point p of device primitive h for a cone of the given width
__device__ __forceinline__ unsigned int proc_word(const float4* prims, const TexView& tv, const ProcView& pv, int h, int prim, int t, int k, V3 p, float width)
{
	const JpProcDev* r = pv.rec + k;
	float2 uv = make_float2(0.f, 0.f);
	if (r->space == JP_PROC_SPACE_UV) uv = tex_uv(prims, tv, h, prim, p);
	const float4 co = tv.col[2 * t], ce = tv.col[2 * t + 1];              // CHECKER: odd, even
	const float c_odd[3] = { co.x, co.y, co.z }, c_even[3] = { ce.x, ce.y, ce.z }, pp[3] = { p.x, p.y, p.z };
	float tt;
	return jp_proc_lookup(r, c_even, c_odd, t, pp, uv.x, uv.y, width, &tt);
}

// tex_sample_m under the records: a texture with a record takes include/jp_procedural.h's lookup, an image with a pyramid (mv.tex may be null: none) tex_sample_m,
// everything else tex_sample_s
__device__ __forceinline__ unsigned int proc_sample(const float4* prims, const TexView& tv, const SampView& sm, const MipView& mv, const ProcView& pv, int h, int prim, int t, V3 p, float width)
{
	const int k = pv.tex[t];
	if (k >= 0) return proc_word(prims, tv, pv, h, prim, t, k, p, width);
	if (mv.tex) { float rho; return tex_sample_m(prims, tv, sm, mv, h, prim, t, p, width, rho); }
	return tex_sample_s(tv, sm.tex, t, tex_uv(prims, tv, h, prim, p), p);
}

// one hit of a path: the cone's step (every hit, where the context carries cones), then the side word (textured hits; 0 else).  Without cones the width is 0.
__device__ __forceinline__ unsigned int proc_hit(const SceneView& sc, const TexView& tv, const SampView& sm, const MipView& mv, const ProcView& pv, bool cone, int h, V3 ro, V3 rd, float thit, int flags, float2& st)
{
	if (cone) jp_mip_cone_hit(mv.gamma0, mv.bounce_spread, flags, thit, &st.x, &st.y);
	const int4 meta = sc.meta[h];
	const int t = meta.y >= 0 ? tv.mat_tex[meta.y] : -1;
	if (t < 0) return 0u;
	const V3 p = ro + thit * rd;                                           // ray(distance), as k_shade forms it
	return proc_sample(sc.prims, tv, sm, mv, pv, h, meta.x, t, p, cone ? st.x : 0.f);
}
} // namespace jp
#endif // JP_PROCEDURAL_DEVICE_PART

#if defined(JP_PROCEDURAL_KERNELS) && !defined(JP_PROCEDURAL_KERNELS_PART)
#define JP_PROCEDURAL_KERNELS_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------------
// k_texel_p: k_texel_m's twin for a scene with at least one procedural record.  Everything k_texel_m does -- the cone's step on every hit through the slot the ray
// carries, pyramids where the scene has them, sampling records -- plus the records' lookups.  mv.cone is null when no procedural is antialiased and the scene has no
// pyramid (every width is 0 then); mv.tex is null when the scene has no pyramid.  The octave loop diverges per lane by design: a lane whose footprint has swallowed
// the remaining octaves leaves it.  Launch bounds as k_texel_m's: four workgroups per CU leave it the registers of two sets of taps, or of an octave's eight corners.
__global__ void __launch_bounds__(JP_BLOCK, 4) k_texel_p(SceneView sc, Queues q, int cur, TexView tv, SampView sm, MipView mv, ProcView pv)
{
	const unsigned int b = blockIdx.x, n = q.blk_q[cur][b], rbase = b * q.R;
	const bool cone = mv.cone != nullptr;
	for (unsigned int j = threadIdx.x; j < n; j += JP_BLOCK)
	{
		const unsigned int i = rbase + j;
		const float2 h = q.hit[i];
		const int pi = __float_as_int(h.y);
		unsigned int w = 0u;
		if (pi >= 0)
		{
			const float4 ro = q.ray_o[cur][i], rd = q.ray_d[cur][i];
			const unsigned int slot = (unsigned int)__float_as_int(ro.w);
			if (slot < q.cap)                                                   // (always: a slot is a position of the batch, and the cone array has cap entries)
			{
				float2 st = make_float2(0.f, 0.f);
				if (cone) st = mv.cone[slot];
				w = proc_hit(sc, tv, sm, mv, pv, cone, pi, xyz(ro), xyz(rd), h.x, __float_as_int(rd.w), st);
				if (cone) mv.cone[slot] = st;
			}
		}
		tv.side[i] = w;
	}
}

// k_proc_probe (jp_procedural_probe): proc_word's lookup on the caller's points, one thread per point; k: the texture's record
__global__ void __launch_bounds__(JP_BLOCK) k_proc_probe(TexView tv, ProcView pv, int texture, int k, int n, const float* p, const float* uv, const float* width, unsigned int* word)
{
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const float4 co = tv.col[2 * texture], ce = tv.col[2 * texture + 1];
		const float c_odd[3] = { co.x, co.y, co.z }, c_even[3] = { ce.x, ce.y, ce.z }, pp[3] = { p[3 * i], p[3 * i + 1], p[3 * i + 2] };
		float tt;
		word[i] = jp_proc_lookup(pv.rec + k, c_even, c_odd, texture, pp, uv[2 * i], uv[2 * i + 1], width[i], &tt);
	}
}

// k_surface_p (jp_surface on a scene with a procedural record): k_surface, with the record's lookup at width 0 -- jp_surface has no cone
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_surface_p(SceneView sc, TexView tv, int depth, int n, const float* o, const float* d, const float* tmin, const float* tmax_in,
                                                        int* prim, float* uv, float* albedo, SampView sm, ProcView pv)
{
	SceneAccess<kMode> acc(sc, depth);
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
		float tmax = tmax_in[i];
		const int h = acc.template trace<false>(sc, ro, rd, tmin[i], tmax);
		float2 st = make_float2(0.f, 0.f); V3 a = splat(0);
		prim[i] = -1;
		if (h >= 0)
		{
			const int4 meta = sc.meta[h];
			const V3 p = ro + tmax * rd;
			prim[i] = meta.x;
			st = tex_uv(sc.prims, tv, h, meta.x, p);
			const int mat = meta.y;
			if (mat >= 0)
			{
				const int mtype = sc.mat_type[mat];
				const int t = tv.mat_tex ? tv.mat_tex[mat] : -1;
				if (t >= 0) { const int k = pv.tex[t]; a = tex_color(tv, k >= 0 ? proc_word(sc.prims, tv, pv, h, meta.x, t, k, p, 0.f) : tex_sample_s(tv, sm.tex, t, st, p)); }
				else if (mtype == JP_MAT_MATTE || mtype == JP_MAT_MIRROR || mtype == JP_MAT_PLASTIC) a = xyz(sc.mats[4 * mat]);
			}
		}
		uv[2 * i] = st.x; uv[2 * i + 1] = st.y;
		albedo[3 * i] = a.x; albedo[3 * i + 1] = a.y; albedo[3 * i + 2] = a.z;
	}
}
#endif // JP_PROCEDURAL_KERNELS

#if defined(JP_PROCEDURAL_RUNTIME) && !defined(JP_PROCEDURAL_RUNTIME_PART)
#define JP_PROCEDURAL_RUNTIME_PART
// ---- part 3: host ---------------------------------------------------------------------------------------------------------------------------
namespace
{
// every rule of a record list, and with `t` the rules that need the textures; n_on: records that are not NONE, n_aa: those of them with antialias on
int check_texture_procedurals(const char* who, const JpTextureProcedurals* v, const JpTextures* t, int& n_on, int& n_aa)
{
	n_on = n_aa = 0;
	if (v->struct_bytes < (int32_t)sizeof(JpTextureProcedurals)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": set JpTextureProcedurals.struct_bytes to sizeof(JpTextureProcedurals)");
	if (v->n_textures < 0 || v->n_textures > (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": n_textures out of range");
	if (t && t->n_textures != v->n_textures) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": n_textures (" + std::to_string(v->n_textures) + ") differs from the textures' (" + std::to_string(t->n_textures) + ")");
	if (!v->rec) return JP_OK;
	for (int i = 0; i < v->n_textures; i++)
	{
		const JpProcedural& r = v->rec[i];
		int rule = jp_procedural_check(&r);
		if (!rule && r.kind != JP_PROC_NONE && t)
		{
			if (!t->tex_type || !t->tex_color) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": null tex_type / tex_color");
			if (t->tex_type[i] != JP_TEXTURE_CHECKER) rule = 9;
			else
			{
				for (int k = 0; k < 6; k++) { const float c = t->tex_color[6 * (size_t)i + k]; if (!(c >= 0.f && c <= 1.f)) rule = 10; }
				if (!rule && r.space == JP_PROC_SPACE_UV && t->n_triangles > 0 && !t->tri_uv) rule = 11;
			}
		}
		if (rule) return fail(JP_ERR_INVALID_ARGUMENT, std::string(who) + ": texture " + std::to_string(i) + ": " + jp_procedural_rule(rule));
		if (r.kind != JP_PROC_NONE) { n_on++; if (r.antialias >= 0) n_aa++; }
	}
	return JP_OK;
}
}

// what the next upload must agree with, checked BEFORE the old scene goes (jp_upload_scene): a refused upload leaves the context with the scene it had
static int check_procedural_counts(const JpContext* c, int n_textures)
{
	const ProceduralsHost& h = c->procedurals;
	if (h.set && h.n_textures != n_textures) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the texture procedurals' n_textures (" + std::to_string(h.n_textures) + ") differs from the upload's (" + std::to_string(n_textures) + ") (jp_set_texture_procedurals)");
	return JP_OK;
}
// ... and the rules that need the textures: a record sits on a CHECKER whose colours lie in [0, 1], and SPACE_UV has the triangles' uv
static int check_procedural_textures(const JpContext* c, const JpTextures* t)
{
	const ProceduralsHost& h = c->procedurals;
	if (!h.set || h.n_on == 0 || t->n_textures != h.n_textures) return JP_OK;     // (a differing count: check_procedural_counts refuses it)
	JpTextureProcedurals v = { (int32_t)sizeof(JpTextureProcedurals), h.n_textures, h.rec.data() };
	int a, b;
	return check_texture_procedurals("jp_upload_scene_textured (jp_set_texture_procedurals)", &v, t, a, b);
}

// The upload's step (jp_upload_scene_textured, a scene with a textured material), after the pyramids: the records of the textures a material uses.  Where an
// antialiased record meets a scene without pyramids the cone's constants are set here as upload_mipmaps sets them (mv.tex stays null).
static int upload_procedurals(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const JpTextures* t)
{
	const ProceduralsHost& h = c->procedurals;
	if (!h.set || h.n_on == 0) return JP_OK;
	std::vector<int> tex((size_t)t->n_textures, -1);
	std::vector<JpProcDev> rec;
	int n_aa = 0;
	for (int m = 0; m < t->n_materials; m++)
	{
		const int k = t->mat_texture[m];
		if (k < 0 || k >= t->n_textures || tex[k] >= 0 || h.rec[k].kind == JP_PROC_NONE) continue;
		tex[k] = (int)rec.size(); rec.push_back(jp_proc_resolve(&h.rec[k]));
		if (h.rec[k].antialias >= 0) n_aa++;
	}
	if (rec.empty()) return JP_OK;                                      // records only on textures no material uses: the upload without them
	HIP_TRY(upload(T.proc_rec, rec.data(), rec.size() * sizeof(JpProcDev)));
	HIP_TRY(upload(T.proc_tex, tex.data(), tex.size() * sizeof(int)));
	plan.proc.rec = T.proc_rec.get<JpProcDev>(); plan.proc.tex = T.proc_tex.get<int>();
	plan.proc_on = (int)rec.size(); plan.proc_aa = n_aa; plan.proc_bytes = (long long)(rec.size() * sizeof(JpProcDev) + tex.size() * sizeof(int));
	if (plan.mip_on == 0) plan.mv = mip_cone_constants(c, s);          // (jp_mipmap.h: the one place that forms gamma0 and the bounce spread)
	return JP_OK;
}

extern "C" {

int jp_check_texture_procedurals(const JpTextureProcedurals* v, const JpTextures* t, int32_t* n_procedural, int32_t* n_antialiased)
{
	if (!v) return fail(JP_ERR_INVALID_ARGUMENT, "jp_check_texture_procedurals: null argument");
	int a, b;
	const int st = check_texture_procedurals("jp_set_texture_procedurals", v, t, a, b);
	if (st == JP_OK) { if (n_procedural) *n_procedural = a; if (n_antialiased) *n_antialiased = b; }
	return st;
}

int jp_set_texture_procedurals(JpContext* c, const JpTextureProcedurals* v)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_procedurals: null context");
	if (!v) { c->procedurals = ProceduralsHost(); return JP_OK; }
	int a, b;
	if (const int st = check_texture_procedurals("jp_set_texture_procedurals", v, nullptr, a, b); st != JP_OK) return st;
	ProceduralsHost h;
	h.set = true; h.n_textures = v->n_textures; h.n_on = a; h.n_aa = b;
	JpProcedural none; std::memset(&none, 0, sizeof(none));
	h.rec.assign((size_t)v->n_textures, none);
	if (v->rec && v->n_textures > 0) h.rec.assign(v->rec, v->rec + v->n_textures);
	c->procedurals = std::move(h);                                     // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_procedural_info(JpContext* c, JpProceduralInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_procedural_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_procedural_info: set JpProceduralInfo.struct_bytes to sizeof(JpProceduralInfo)");
	JpProceduralInfo i; std::memset(&i, 0, sizeof(i));
	if (c->plan.have_scene && c->plan.proc_on > 0) { i.n_procedural = c->plan.proc_on; i.n_antialiased = c->plan.proc_aa; i.table_bytes_device = c->plan.proc_bytes; }
	i.procedural_last_render = c->last_proc;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_procedural_lookup(const JpProcedural* rec, const float* c_even, const float* c_odd, int32_t texture, int32_t n, const float* p, const float* uv, const float* width,
                         uint32_t* word_out, float* t_out)
{
	if (!rec || !c_even || !c_odd || n < 0 || (n > 0 && (!p || !uv || !width))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_lookup: null argument");
	if (texture < 0 || texture >= (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_lookup: texture out of range");
	if (const int r = jp_procedural_check(rec)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_procedural_lookup: ") + jp_procedural_rule(r));
	if (rec->kind == JP_PROC_NONE) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_lookup: the record's kind is JP_PROC_NONE");
	const JpProcDev d = jp_proc_resolve(rec);
	for (int32_t i = 0; i < n; i++)
	{
		float t;
		const unsigned int w = jp_proc_lookup(&d, c_even, c_odd, texture, p + 3 * (size_t)i, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], width[i], &t);
		if (word_out) word_out[i] = w;
		if (t_out) t_out[i] = t;
	}
	return JP_OK;
}

int jp_procedural_probe(JpContext* c, int32_t texture, int32_t n, const float* p, const float* uv, const float* width, uint32_t* word_out)
{
	if (!c || n < 0 || !p || !uv || !width || !word_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_probe: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_procedural_probe: no scene uploaded");
	if (c->plan.proc_on == 0) return fail(JP_ERR_UNSUPPORTED, "jp_procedural_probe: the uploaded scene has no procedural record (jp_set_texture_procedurals)");
	if (texture < 0 || texture >= c->n_textures) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_probe: texture out of range");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	int k = -1;
	HIP_TRY(hipMemcpy(&k, c->plan.proc.tex + texture, sizeof(int), hipMemcpyDeviceToHost));
	if (k < 0 || k >= c->plan.proc_on) return fail(JP_ERR_INVALID_ARGUMENT, "jp_procedural_probe: texture " + std::to_string(texture) + " has no procedural record");
	DevBuf b_in, b_out; float* d_in; unsigned int* d_w;                 // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 24)); HIP_TRY(reserve(b_out, d_w, (size_t)n * 4));
	float *d_p = d_in, *d_uv = d_in + 3 * (size_t)n, *d_wd = d_in + 5 * (size_t)n;
	HIP_TRY(hipMemcpyAsync(d_p, p, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_uv, uv, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_wd, width, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::max(1, std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK));
	hipLaunchKernelGGL(k_proc_probe, dim3(grid), dim3(JP_BLOCK), 0, c->stream, c->plan.tv, c->plan.proc, (int)texture, k, (int)n, d_p, d_uv, d_wd, d_w);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(word_out, d_w, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return JP_OK;
}

} // extern "C"
#endif // JP_PROCEDURAL_RUNTIME
