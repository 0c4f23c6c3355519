// jet-pbrt_amd/csrc/jp_tex_sampling.h -- texture sampling records (INTEGRATION.md "Texture sampling", DESIGN.md "Texture sampling"), in three parts:
//   part 1 (included by jp_normal_map.h's part 1, before mapped_normal): SampView and tex_sample_s, the device side of include/jp_tex_sampling.h
//   part 2 (JP_TEX_SAMPLING_KERNELS, after the kernels): k_texel_s and k_normal_map_s, the twins a scene with an active record runs in k_texel's / k_normal_map's place
//   part 3 (JP_TEX_SAMPLING_RUNTIME, at the end): the upload's table steps and the entry points jp_set_texture_sampling / jp_check_texture_sampling /
//     jp_get_texture_sampling_info / jp_texture_lookup / jp_perturb_normals_sampled.
// The records change what the side kernels WRITE, never the record's layout: k_shade and its families read the same 32-bit word and the same 16-byte normal record.
// A context without an active record runs nothing of this file.
#ifndef JP_TEX_SAMPLING_DEVICE_PART
#define JP_TEX_SAMPLING_DEVICE_PART
#include "jp_common.h"
#include "jp_tex.h"
#include "../../include/jp_tex_sampling.h"

// ---- part 1 -----------------------------------------------------------------------------------------------------------------------------
// one 32-byte slot per texture / per map, read uniformly per texture; active 0: the identity, the lookup without records
struct SampSlot { JpTexSampler s; int32_t active; };
// A separate kernel argument of the side kernels, the hooks and the guides only: TexView and NMapView stay as they are, k_shade_tex* takes TexView by value.
struct SampView
{
	const SampSlot* tex;         // per texture of TexView::desc; null: no active colour record
	const SampSlot* map;         // per map of NMapView::desc; null: no active normal-map record
};

namespace jp
{
// tex_sample under the records: an image texture with an active record takes include/jp_tex_sampling.h's lookup, everything else tex_sample
__device__ __forceinline__ unsigned int tex_sample_s(const TexView& tv, const SampSlot* slots, int t, float2 uv, V3 p)
{
	if (slots)
	{
		const int4 d = tv.desc[t];
		const SampSlot sl = slots[t];
		if (d.x == JP_TEXTURE_IMAGE && sl.active) return JP_TEX_IMAGE_TAG | jp_tex_lookup_sampled(&sl.s, tv.texels + (size_t)d.w, d.y, d.z, uv.x, uv.y);
	}
	return tex_sample(tv, t, uv, p);
}
} // namespace jp
#endif // JP_TEX_SAMPLING_DEVICE_PART

#if defined(JP_TEX_SAMPLING_KERNELS) && !defined(JP_TEX_SAMPLING_KERNELS_PART)
#define JP_TEX_SAMPLING_KERNELS_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------------
// k_texel_s: k_texel's twin for a scene with at least one active colour record.  The same dependent gather (hit -> primitive record -> material -> descriptor), then the
// texture's slot and, for a bilinear record, four texel loads issued together: one more round trip than k_texel whatever the filter.  Same side word.
__global__ void __launch_bounds__(JP_BLOCK, 8) k_texel_s(SceneView sc, Queues q, int cur, TexView tv, SampView sm)
{
	const unsigned int b = blockIdx.x, n = q.blk_q[cur][b], rbase = b * q.R;
	for (unsigned int j = threadIdx.x; j < n; j += JP_BLOCK)
	{
		const unsigned int i = rbase + j;
		const float2 h = q.hit[i];
		const int pi = __float_as_int(h.y);
		unsigned int w = 0u;
		if (pi >= 0)
		{
			const int4 meta = sc.meta[pi];
			const int t = meta.y >= 0 ? tv.mat_tex[meta.y] : -1;
			if (t >= 0)
			{
				const float4 ro = q.ray_o[cur][i], rd = q.ray_d[cur][i];
				const V3 p = xyz(ro) + h.x * xyz(rd);                               // ray(distance), as k_shade forms it
				w = tex_sample_s(tv, sm.tex, t, tex_uv(sc.prims, tv, pi, meta.x, p), p);
			}
		}
		tv.side[i] = w;
	}
}

// k_normal_map_s: k_normal_map's twin for a scene with at least one active normal-map record; it differs in the lookup's addressing alone
__global__ void __launch_bounds__(JP_BLOCK, 8) k_normal_map_s(SceneView sc, Queues q, int cur, NormView nv, NMapView mp, SampView sm)
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
			const int4 meta = sc.meta[pi];
			const bool has_map = meta.y >= 0 && __float_as_int(mp.mat[meta.y].x) >= 0;
			if (has_map || nv.prim_vn)
			{
				const float4 ro = q.ray_o[cur][i], rd = q.ray_d[cur][i];
				const V3 p = xyz(ro) + h.x * xyz(rd);                                   // ray(distance), as k_shade forms it
				V3 Ns = mk(0, 0, 0);
				bool on = nv.prim_vn && shading_normal(sc.prims, nv, pi, meta.x, p, Ns);
				if (has_map)
				{
					const V3 N = hit_normal(sc.prims, pi, p, xyz(rd));
					if (mapped_normal(sc.prims, mp, pi, meta.x, meta.y, p, N, on ? Ns : N, Ns, sm.map)) on = true;
				}
				if (on) rec = make_float4(Ns.x, Ns.y, Ns.z, 1.f);
			}
		}
		nv.side[i] = rec;
	}
}
#endif // JP_TEX_SAMPLING_KERNELS

#if defined(JP_TEX_SAMPLING_RUNTIME) && !defined(JP_TEX_SAMPLING_RUNTIME_PART)
#define JP_TEX_SAMPLING_RUNTIME_PART
// ---- part 3: host ---------------------------------------------------------------------------------------------------------------------------
namespace
{
// one list of records: every rule of jp_tex_sampler_check with its message; n_active: records that are not the identity
int check_sampler_list(const char* what, int kind, int n, const JpTexSampler* s, int& n_active)
{
	n_active = 0;
	if (n < 0 || n > (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_set_texture_sampling: n_") + (kind == JP_TSAMP_NORMAL ? "maps" : "textures") + " out of range");
	if (!s) return JP_OK;
	for (int i = 0; i < n; i++)
	{
		if (const int r = jp_tex_sampler_check(s + i, kind)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_set_texture_sampling: ") + what + " " + std::to_string(i) + ": " + jp_tex_sampler_rule(r));
		if (!jp_tsamp_identity(s + i, kind)) n_active++;
	}
	return JP_OK;
}
int check_texture_sampling(const JpTextureSampling* t, int& na_tex, int& na_map)
{
	na_tex = na_map = 0;
	if (t->struct_bytes < (int32_t)sizeof(JpTextureSampling)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_sampling: set JpTextureSampling.struct_bytes to sizeof(JpTextureSampling)");
	if (const int st = check_sampler_list("texture", JP_TSAMP_COLOR, t->n_textures, t->tex, na_tex); st != JP_OK) return st;
	return check_sampler_list("normal map", JP_TSAMP_NORMAL, t->n_maps, t->map, na_map);
}
std::vector<SampSlot> sampler_slots(const std::vector<JpTexSampler>& s, int kind)
{
	std::vector<SampSlot> v(s.size());
	for (size_t i = 0; i < s.size(); i++) { v[i].s = s[i]; v[i].active = jp_tsamp_identity(&s[i], kind) ? 0 : 1; }
	return v;
}
}

// what the next upload must agree with, checked BEFORE the old scene goes (jp_upload_scene): a refused upload leaves the context with the scene it had
static int check_sampling_counts(const JpContext* c, int n_textures)
{
	const TexSamplingHost& h = c->tsamp;
	if (h.has_tex && h.n_textures != n_textures) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the texture sampling's n_textures (" + std::to_string(h.n_textures) + ") differs from the upload's (" + std::to_string(n_textures) + ") (jp_set_texture_sampling)");
	const int nm = c->nmaps.set ? (int)c->nmaps.width.size() : 0;
	if (h.has_map && h.n_maps != nm) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the texture sampling's n_maps (" + std::to_string(h.n_maps) + ") differs from the normal maps' (" + std::to_string(nm) + ") (jp_set_texture_sampling)");
	return JP_OK;
}
// ... and a record that is not the identity addresses an image
static int check_sampling_textures(const JpContext* c, const JpTextures* t)
{
	const TexSamplingHost& h = c->tsamp;
	if (!h.has_tex) return JP_OK;
	for (int i = 0; i < t->n_textures && i < h.n_textures; i++)
		if (t->tex_type[i] != JP_TEXTURE_IMAGE && !jp_tsamp_identity(&h.tex[i], JP_TSAMP_COLOR))
			return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: texture " + std::to_string(i) + ": a sampling record on a solid or checker texture (jp_set_texture_sampling)");
	return JP_OK;
}

// the upload's table steps: the slots of the maps (jp_upload_scene, after upload_normal_maps, for a scene whose maps perturb) and of the textures
// (jp_upload_scene_textured, for a scene with a textured material) -- only where a record is active
static int upload_map_sampling(JpContext* c, SceneTables& T, ScenePlan& plan)
{
	const TexSamplingHost& h = c->tsamp;
	if (!h.has_map || h.n_active_maps == 0 || !plan.mapped) return JP_OK;
	const std::vector<SampSlot> v = sampler_slots(h.map, JP_TSAMP_NORMAL);
	HIP_TRY(upload(T.ts_map, v.data(), v.size() * sizeof(SampSlot)));
	plan.sm.map = T.ts_map.get<SampSlot>(); plan.ts_active_maps = h.n_active_maps; plan.ts_table_bytes += (long long)(v.size() * sizeof(SampSlot));
	return JP_OK;
}
static int upload_tex_sampling(JpContext* c, SceneTables& T, ScenePlan& plan)
{
	const TexSamplingHost& h = c->tsamp;
	if (!h.has_tex || h.n_active_textures == 0 || !plan.textured) return JP_OK;
	const std::vector<SampSlot> v = sampler_slots(h.tex, JP_TSAMP_COLOR);
	HIP_TRY(upload(T.ts_tex, v.data(), v.size() * sizeof(SampSlot)));
	plan.sm.tex = T.ts_tex.get<SampSlot>(); plan.ts_active_textures = h.n_active_textures; plan.ts_table_bytes += (long long)(v.size() * sizeof(SampSlot));
	return JP_OK;
}

extern "C" {

int jp_check_texture_sampling(const JpTextureSampling* t, int32_t* n_active_textures, int32_t* n_active_maps)
{
	if (!t) return fail(JP_ERR_INVALID_ARGUMENT, "jp_check_texture_sampling: null argument");
	int a, b;
	const int st = check_texture_sampling(t, a, b);
	if (st == JP_OK) { if (n_active_textures) *n_active_textures = a; if (n_active_maps) *n_active_maps = b; }
	return st;
}

int jp_set_texture_sampling(JpContext* c, const JpTextureSampling* t)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_sampling: null context");
	if (!t) { c->tsamp = TexSamplingHost(); return JP_OK; }
	int a, b;
	if (const int st = check_texture_sampling(t, a, b); st != JP_OK) return st;
	TexSamplingHost h;
	h.has_tex = t->tex != nullptr; h.has_map = t->map != nullptr; h.n_textures = t->n_textures; h.n_maps = t->n_maps; h.n_active_textures = a; h.n_active_maps = b;
	if (t->tex && t->n_textures > 0) h.tex.assign(t->tex, t->tex + t->n_textures);
	if (t->map && t->n_maps > 0) h.map.assign(t->map, t->map + t->n_maps);
	c->tsamp = std::move(h);                                           // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_texture_sampling_info(JpContext* c, JpTexSamplingInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_sampling_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_sampling_info: set JpTexSamplingInfo.struct_bytes to sizeof(JpTexSamplingInfo)");
	JpTexSamplingInfo i; std::memset(&i, 0, sizeof(i));
	if (c->plan.have_scene) { i.n_active_textures = c->plan.ts_active_textures; i.n_active_maps = c->plan.ts_active_maps; i.table_bytes_device = c->plan.ts_table_bytes; }
	i.sampled_last_render = c->last_sampled;
	if (c->profiling && (c->last_textured || c->last_nmapped))
	{   // the side kernels' launches of the last render, all lanes (HIP-event times; synchronises)
		if (const int st = finish_counters(c); st != JP_OK) return st;
		i.texel_ms = c->texel_ms; i.normal_map_ms = c->normal_map_ms;
		for (int k = 1; k < c->last_lanes; k++) { i.texel_ms += c->lanes[k - 1]->texel_ms; i.normal_map_ms += c->lanes[k - 1]->normal_map_ms; }
	}
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_texture_lookup(const JpTexSampler* s, int32_t w, int32_t h, const uint8_t* rgb8, int32_t n, const float* uv, uint8_t* rgb8_out)
{
	if (n < 0 || (n > 0 && (!uv || !rgb8_out)) || !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_texture_lookup: null argument");
	if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_texture_lookup: size out of range (1 .. 16384 per side)");
	if (s) if (const int r = jp_tex_sampler_check(s, JP_TSAMP_COLOR)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_texture_lookup: ") + jp_tex_sampler_rule(r));
	std::vector<unsigned int> texels((size_t)w * (size_t)h);
	pack_rgb8(rgb8, texels.size(), texels.data());
	const bool active = s && !jp_tsamp_identity(s, JP_TSAMP_COLOR);
	for (int32_t i = 0; i < n; i++)
	{
		const float u = uv[2 * (size_t)i], v = uv[2 * (size_t)i + 1];
		const unsigned int t = active ? jp_tex_lookup_sampled(s, texels.data(), w, h, u, v) : (texels[jp_tsamp_nearest_clamp(w, h, u, v)] & 0xffffffu);
		rgb8_out[3 * (size_t)i] = (uint8_t)(t & 0xffu); rgb8_out[3 * (size_t)i + 1] = (uint8_t)((t >> 8) & 0xffu); rgb8_out[3 * (size_t)i + 2] = (uint8_t)((t >> 16) & 0xffu);
	}
	return JP_OK;
}

int jp_perturb_normals_sampled(const JpTexSampler* s, int32_t n, const float* nb, const float* ng, const float* dpdu, const float* dpdv, const float* uv,
                               int32_t width, int32_t height, const uint8_t* rgb8, float strength, float* ns_out, int32_t* perturbed_out)
{
	if (!s || jp_tsamp_identity(s, JP_TSAMP_NORMAL)) return jp_perturb_normals(n, nb, ng, dpdu, dpdv, uv, width, height, rgb8, strength, ns_out, perturbed_out);
	if (const int r = jp_tex_sampler_check(s, JP_TSAMP_NORMAL)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_perturb_normals_sampled: ") + jp_tex_sampler_rule(r));
	if (n < 0 || (n > 0 && (!nb || !ng || !dpdu || !dpdv || !uv || !ns_out || !perturbed_out)) || !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_perturb_normals_sampled: null argument");
	if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_perturb_normals_sampled: size out of range (1 .. 16384 per side)");
	std::vector<unsigned int> texels((size_t)width * (size_t)height);
	pack_rgb8(rgb8, texels.size(), texels.data());
	for (int32_t i = 0; i < n; i++)
	{
		const size_t k = 3 * (size_t)i;
		float ns[3] = { nb[k], nb[k + 1], nb[k + 2] };                  // unperturbed: the base normal
		perturbed_out[i] = jp_perturb_normal_sampled(s, nb + k, ng + k, dpdu + k, dpdv + k, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], texels.data(), width, height, strength, ns);
		ns_out[k] = ns[0]; ns_out[k + 1] = ns[1]; ns_out[k + 2] = ns[2];
	}
	return JP_OK;
}

} // extern "C"
#endif // JP_TEX_SAMPLING_RUNTIME
