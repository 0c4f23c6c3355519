// jet-pbrt_amd/csrc/jp_mipmap.h -- mip-mapped image textures (INTEGRATION.md "Mip maps", DESIGN.md "Mip maps"), in three parts like jp_tex_sampling.h:
//   part 1 (after the kernels and jp_tex_sampling.h's part 2): MipView and tex_sample_m, the device side of include/jp_mipmap.h
//   part 2 (JP_MIPMAP_KERNELS, right after part 1): k_mip_level (the upload's pyramid builder), k_texel_m (k_texel_s's twin for a scene with at least one pyramid) and
//     the test hook k_mip_probe
//   part 3 (JP_MIPMAP_RUNTIME, at the end): the upload's steps and the entry points jp_set_texture_mipmaps / jp_check_texture_mipmaps / jp_get_texture_mipmap_info /
//     jp_read_mip_chain / jp_build_mip_chain / jp_mip_cone_step / jp_mip_footprint / jp_texture_lookup_mip / jp_mip_probe.
// Mip maps change what the side kernel WRITES, never the word's layout: k_shade_tex* read the same 24-bit RGB8 word.  The ray cone is two floats per path slot, read and
// written by k_texel_m alone: a queued ray carries its slot in ray_o.w and its bounce and specular flag in ray_d.w, so no traversal or shading kernel knows of it.
// A context without a pyramid runs nothing of this file.
#ifndef JP_MIPMAP_DEVICE_PART
#define JP_MIPMAP_DEVICE_PART
#include "jp_common.h"
#include "jp_tex.h"
#include "jp_tex_sampling.h"
#include "../../include/jp_mipmap.h"

// ---- part 1 -----------------------------------------------------------------------------------------------------------------------------
// A separate kernel argument of k_texel_m, k_mip_probe and the guides only: TexView, SampView and Queues stay as they are.
struct MipView
{
	float2* cone;                // (width, spread) per path slot of the launching context's queue set; null outside a render (guides, probe)
	const int2* tex;             // per texture of TexView::desc: (first record in lev, levels; 0 levels: no pyramid); null: the scene has no pyramid
	const JpMipLevel* lev;       // (width, height, first texel in TexView::texels, -) per level, level 0 included
	float gamma0, bounce_spread, footprint_scale;
};

namespace jp
{
// A of include/jp_mipmap.h at the point p of device primitive h (caller's primitive index prim)
__device__ __forceinline__ float mip_area(const float4* prims, const TexView& tv, int h, int prim, V3 p)
{
	const float4 g0 = prims[4 * h], g3 = prims[4 * h + 3];
	const int type = __float_as_int(g3.w);
	if (type == JP_SHAPE_TRIANGLE)
	{
		if (!tv.prim_uv) return 0.f;
		const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
		const float2 t0 = tv.prim_uv[3 * prim], t1 = tv.prim_uv[3 * prim + 1], t2 = tv.prim_uv[3 * prim + 2];
		const float a0[3] = { g0.x, g0.y, g0.z }, a1[3] = { g1.x, g1.y, g1.z }, a2[3] = { g2.x, g2.y, g2.z }, uv6[6] = { t0.x, t0.y, t1.x, t1.y, t2.x, t2.y };
		return jp_mip_area_triangle(a0, a1, a2, uv6);
	}
	if (type == JP_SHAPE_RECTANGLE)
	{   // p3 rides in the w components (tex_uv)
		const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
		const float a0[3] = { g0.x, g0.y, g0.z }, a1[3] = { g1.x, g1.y, g1.z }, a3[3] = { g0.w, g1.w, g2.w };
		return jp_mip_area_rectangle(a0, a1, a3);
	}
	const V3 d = p - xyz(g0);
	const float dd[3] = { d.x, d.y, d.z };
	return type == JP_SHAPE_DISK ? jp_mip_area_disk(dd, g0.w) : jp_mip_area_sphere(dd, g0.w);
}

// tex_sample_s under the pyramids: the side word of texture t at the point p of device primitive h for a cone of the given width; rho: the footprint in texels
// (0: the texture has no pyramid).  rho <= 1 takes tex_sample_s itself.
__device__ __forceinline__ unsigned int tex_sample_m(const float4* prims, const TexView& tv, const SampView& sm, const MipView& mv, int h, int prim, int t, V3 p, float width, float& rho)
{
	const float2 uv = tex_uv(prims, tv, h, prim, p);
	rho = 0.f;
	const int2 ml = mv.tex[t];
	if (ml.y > 0)
	{
		const int4 d = tv.desc[t];
		JpTexSampler s = jp_mip_identity_sampler();
		if (sm.tex) { const SampSlot sl = sm.tex[t]; if (sl.active) s = sl.s; }
		rho = jp_mip_rho(width, mip_area(prims, tv, h, prim, p), d.y, d.z, s.scale_u, s.scale_v, mv.footprint_scale);
		if (rho > 1.f) return JP_TEX_IMAGE_TAG | jp_mip_lookup_above(&s, tv.texels, mv.lev + ml.x, ml.y, uv.x, uv.y, rho);
	}
	return tex_sample_s(tv, sm.tex, t, uv, p);
}

// one hit of a path: the cone's step (every hit), then the side word (textured hits; 0 else).  What k_texel_m does per queued ray and k_mip_probe per probe ray.
__device__ __forceinline__ unsigned int mip_hit(const SceneView& sc, const TexView& tv, const SampView& sm, const MipView& mv, int h, V3 ro, V3 rd, float thit, int flags, float2& st, float& rho)
{
	jp_mip_cone_hit(mv.gamma0, mv.bounce_spread, flags, thit, &st.x, &st.y);
	rho = 0.f;
	const int4 meta = sc.meta[h];
	const int t = meta.y >= 0 ? tv.mat_tex[meta.y] : -1;
	if (t < 0) return 0u;
	const V3 p = ro + thit * rd;                                           // ray(distance), as k_shade forms it
	return tex_sample_m(sc.prims, tv, sm, mv, h, meta.x, t, p, st.x, rho);
}
} // namespace jp
#endif // JP_MIPMAP_DEVICE_PART

#if defined(JP_MIPMAP_KERNELS) && !defined(JP_MIPMAP_KERNELS_PART)
#define JP_MIPMAP_KERNELS_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------------
// k_mip_level: one level of one pyramid from the level above it, one thread per texel of the new level (include/jp_mipmap.h, jp_mip_down_texel)
__global__ void __launch_bounds__(JP_BLOCK) k_mip_level(unsigned int* texels, unsigned int src, int sw, int sh, unsigned int dst, int dw, int dh)
{
	const int n = dw * dh;
	for (int k = blockIdx.x * JP_BLOCK + threadIdx.x; k < n; k += gridDim.x * JP_BLOCK)
	{
		const int j = k / dw, i = k - j * dw;
		texels[(size_t)dst + (size_t)k] = jp_mip_down_texel(texels + (size_t)src, sw, sh, i, j);
	}
}

// k_texel_m: k_texel_s's twin for a scene with at least one pyramid.  The same dependent gather, plus the slot's cone -- one 8-byte load and store per hit, textured
// or not, through the slot the ray carries -- and above one texel of footprint two levels' taps, eight texel loads issued together.  Same side word.
// (Held to k_texel_s's 64 registers it spills 28 of them to scratch: two sets of taps and weights are live at once.  Four workgroups per CU leave it the registers.)
__global__ void __launch_bounds__(JP_BLOCK, 4) k_texel_m(SceneView sc, Queues q, int cur, TexView tv, SampView sm, MipView mv)
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
			const float4 ro = q.ray_o[cur][i], rd = q.ray_d[cur][i];
			const unsigned int slot = (unsigned int)__float_as_int(ro.w);
			if (slot < q.cap)                                                   // (always: a slot is a position of the batch, and the cone array has cap entries)
			{
				float2 st = mv.cone[slot];
				float rho;
				w = mip_hit(sc, tv, sm, mv, pi, xyz(ro), xyz(rd), h.x, __float_as_int(rd.w), st, rho);
				mv.cone[slot] = st;
			}
		}
		tv.side[i] = w;
	}
}

// k_mip_probe (jp_mip_probe): the closest hit of k_surface's walk, then mip_hit on the caller's flags and state
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_mip_probe(SceneView sc, TexView tv, SampView sm, MipView mv, int depth, int n, const float* o, const float* d, const float* tmin, const float* tmax_in,
                                                        const int* flags, float* state, int* prim, float* rho_out, unsigned int* word)
{
	SceneAccess<kMode> acc(sc, depth);
	for (int i = blockIdx.x * JP_BLOCK + threadIdx.x; i < n; i += gridDim.x * JP_BLOCK)
	{
		const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
		float tmax = tmax_in[i];
		const int h = acc.template trace<false>(sc, ro, rd, tmin[i], tmax);
		float rho = 0.f; unsigned int w = 0u; int pr = -1;
		if (h >= 0)
		{
			float2 st = make_float2(state[2 * i], state[2 * i + 1]);
			w = mip_hit(sc, tv, sm, mv, h, ro, rd, tmax, flags[i], st, rho);
			state[2 * i] = st.x; state[2 * i + 1] = st.y;
			pr = sc.meta[h].x;
		}
		prim[i] = pr; rho_out[i] = rho; word[i] = w;
	}
}
#endif // JP_MIPMAP_KERNELS

#if defined(JP_MIPMAP_RUNTIME) && !defined(JP_MIPMAP_RUNTIME_PART)
#define JP_MIPMAP_RUNTIME_PART
// ---- part 3: host ---------------------------------------------------------------------------------------------------------------------------
namespace
{
int check_texture_mipmaps(const JpTextureMipmaps* m, int& n_on)
{
	n_on = 0;
	if (m->struct_bytes < (int32_t)sizeof(JpTextureMipmaps)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_mipmaps: set JpTextureMipmaps.struct_bytes to sizeof(JpTextureMipmaps)");
	if (m->n_textures < 0 || m->n_textures > (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_mipmaps: n_textures out of range");
	int bad;
	if (const int r = jp_mipmaps_check(m, &bad, &n_on))
		return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_set_texture_mipmaps: ") + (r == 1 ? "texture " + std::to_string(bad) + ": " : std::string()) + jp_mipmaps_rule(r));
	return JP_OK;
}

// the levels of one image: sizes and first texels relative to the chain's start (level 0 at 0); the chain's texels in all
long long mip_chain_layout(int w, int h, std::vector<JpMipLevel>& lev)
{
	lev.clear();
	long long at = 0;
	const int n = jp_mip_levels(w, h);
	for (int k = 0; k < n; k++)
	{
		JpMipLevel l = { w, h, (int32_t)at, 0 }; lev.push_back(l);
		at += (long long)w * h; w = jp_mip_half(w); h = jp_mip_half(h);
	}
	return at;
}
// the host builder: the chain of one image in dwords, level 0 first
void mip_chain_build(int w, int h, const std::vector<JpMipLevel>& lev, std::vector<unsigned int>& texels)
{
	for (size_t k = 1; k < lev.size(); k++)
		for (int j = 0; j < lev[k].h; j++)
			for (int i = 0; i < lev[k].w; i++)
				texels[(size_t)lev[k].first + (size_t)j * lev[k].w + i] = jp_mip_down_texel(texels.data() + lev[k - 1].first, lev[k - 1].w, lev[k - 1].h, i, j);
}
void unpack_rgb8(const unsigned int* texels, size_t n, uint8_t* rgb8)
{
	for (size_t k = 0; k < n; k++) { rgb8[3 * k] = (uint8_t)(texels[k] & 0xffu); rgb8[3 * k + 1] = (uint8_t)((texels[k] >> 8) & 0xffu); rgb8[3 * k + 2] = (uint8_t)((texels[k] >> 16) & 0xffu); }
}
// the textures of an upload whose pyramid is built: mode TRILINEAR and used by a material
std::vector<char> mip_textures_on(const MipmapsHost& h, const JpTextures* t)
{
	std::vector<char> on((size_t)std::max(0, t->n_textures), 0);
	if (!h.set || h.n_on == 0) return on;
	for (int m = 0; m < t->n_materials; m++) { const int k = t->mat_texture[m]; if (k >= 0 && k < t->n_textures && k < (int)h.mode.size() && h.mode[k] == JP_MIP_TRILINEAR) on[k] = 1; }
	return on;
}
}

// what the next upload must agree with, checked BEFORE the old scene goes (jp_upload_scene): a refused upload leaves the context with the scene it had
static int check_mipmap_counts(const JpContext* c, int n_textures)
{
	const MipmapsHost& h = c->mipmaps;
	if (h.set && h.n_textures != n_textures) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the texture mipmaps' n_textures (" + std::to_string(h.n_textures) + ") differs from the upload's (" + std::to_string(n_textures) + ") (jp_set_texture_mipmaps)");
	return JP_OK;
}
// ... a mode that is not OFF addresses an image, and the pool with its pyramids stays below 2^31 texels (the descriptors' int offsets)
static int check_mipmap_textures(const JpContext* c, const JpTextures* t, long long pool)
{
	const MipmapsHost& h = c->mipmaps;
	if (!h.set) return JP_OK;
	for (int i = 0; i < t->n_textures && i < h.n_textures; i++)
		if (t->tex_type[i] != JP_TEXTURE_IMAGE && h.mode[i] != JP_MIP_OFF)
			return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: texture " + std::to_string(i) + ": mipmaps on a solid or checker texture (jp_set_texture_mipmaps)");
	const std::vector<char> on = mip_textures_on(h, t);
	std::vector<JpMipLevel> lev;
	for (int i = 0; i < t->n_textures; i++) if (on[i]) pool += mip_chain_layout(t->tex_width[i], t->tex_height[i], lev) - (long long)t->tex_width[i] * t->tex_height[i];
	if (pool > 0x7fffffffll) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: more than 2^31 texels in all with the pyramids (jp_set_texture_mipmaps)");
	return JP_OK;
}

// The upload's steps (jp_upload_scene_textured, a scene with a textured material).  mip_reserve_pool, before the texel pool is copied up: the pool's allocation
// grows by the pyramids.  upload_mipmaps, after it: the level tables, then one k_mip_level launch per level.
static long long mip_pool_texels(const JpContext* c, const JpTextures* t, long long pool)
{
	const std::vector<char> on = mip_textures_on(c->mipmaps, t);
	std::vector<JpMipLevel> lev;
	for (int i = 0; i < t->n_textures; i++) if (on[i]) pool += mip_chain_layout(t->tex_width[i], t->tex_height[i], lev) - (long long)t->tex_width[i] * t->tex_height[i];
	return pool;
}
// the cone's constants of an upload, defaults resolved: what upload_mipmaps and upload_procedurals (jp_procedural.h: an antialiased record on a scene without
// pyramids carries cones too) put into the plan's MipView; tex / lev / cone stay null
static MipView mip_cone_constants(const JpContext* c, const JpScene* s)
{
	const MipmapsHost& h = c->mipmaps;
	MipView mv = MipView();
	mv.footprint_scale = h.set && h.footprint_scale != 0.f ? h.footprint_scale : 1.f;
	mv.bounce_spread = h.set && h.bounce_spread != 0.f ? h.bounce_spread : JP_MIP_DEFAULT_BOUNCE_SPREAD;
	const float* up = s->camera.up;
	mv.gamma0 = 2.f * sqrtf((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]) / s->camera.res_y;
	return mv;
}
static int upload_mipmaps(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s, const JpTextures* t, const std::vector<int4>& desc, long long pool)
{
	const MipmapsHost& h = c->mipmaps;
	const std::vector<char> on = mip_textures_on(h, t);
	int n_on = 0; for (const char v : on) n_on += v;
	if (n_on == 0) return JP_OK;
	std::vector<int2> tex((size_t)t->n_textures, make_int2(0, 0));
	std::vector<JpMipLevel> all, lev;
	long long at = pool;
	for (int i = 0; i < t->n_textures; i++)
	{
		if (!on[i]) continue;
		mip_chain_layout(desc[i].y, desc[i].z, lev);
		tex[i] = make_int2((int)all.size(), (int)lev.size());
		for (size_t k = 0; k < lev.size(); k++)
		{
			JpMipLevel l = lev[k];
			if (k == 0) l.first = desc[i].w; else { l.first = (int32_t)at; at += (long long)l.w * l.h; }
			all.push_back(l);
		}
	}
	if ((size_t)at * sizeof(unsigned int) > T.texels.bytes()) return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: the texel pool was not grown by the pyramids");
	HIP_TRY(upload(T.mip_tex, tex.data(), tex.size() * sizeof(int2)));
	HIP_TRY(upload(T.mip_lev, all.data(), all.size() * sizeof(JpMipLevel)));
	hipEvent_t e0 = nullptr, e1 = nullptr;
	HIP_TRY(hipEventCreate(&e0)); if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: event allocation failed"); }
	hipEventRecord(e0, c->stream);
	unsigned int* const d_texels = T.texels.get<unsigned int>();
	for (int i = 0; i < t->n_textures; i++)
		for (int k = 1; k < tex[i].y; k++)
		{   // (in stream order: level k reads level k - 1)
			const JpMipLevel& a = all[(size_t)tex[i].x + k - 1]; const JpMipLevel& b = all[(size_t)tex[i].x + k];
			const int grid = std::max(1, std::min(c->n_cus * 8, (b.w * b.h + JP_BLOCK - 1) / JP_BLOCK));
			hipLaunchKernelGGL(k_mip_level, dim3(grid), dim3(JP_BLOCK), 0, c->stream, d_texels, (unsigned int)a.first, a.w, a.h, (unsigned int)b.first, b.w, b.h);
		}
	hipEventRecord(e1, c->stream);
	const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(c->stream);
	float ms = 0.f; if (le == hipSuccess && se == hipSuccess) hipEventElapsedTime(&ms, e0, e1);
	hipEventDestroy(e0); hipEventDestroy(e1);
	HIP_TRY(le); HIP_TRY(se);
	MipView& mv = plan.mv; mv = mip_cone_constants(c, s);
	mv.tex = T.mip_tex.get<int2>(); mv.lev = T.mip_lev.get<JpMipLevel>();
	plan.mip_on = n_on; plan.mip_levels = (int)all.size();
	plan.mip_bytes = (at - pool) * 4 + (long long)(tex.size() * sizeof(int2) + all.size() * sizeof(JpMipLevel));
	c->mip_build_ms = ms; c->mip_host_tex = std::move(tex); c->mip_host_lev = std::move(all);
	return JP_OK;
}

// the cone array of a context's queue set: one float2 per path slot, allocated by the first render that needs it
static int ensure_cone(JpContext* c, unsigned int cap, MipView& mv)
{
	if (const int e = reserve_idle(c, c->cone, (size_t)cap * sizeof(float2)); e != JP_OK) return e;
	mv.cone = c->cone.get<float2>();
	return JP_OK;
}

typedef void (*MipProbeKernel)(SceneView, TexView, SampView, MipView, int, int, const float*, const float*, const float*, const float*, const int*, float*, int*, float*, unsigned int*);
struct MipProbeOf { template <class M> MipProbeKernel operator()(M) const { return k_mip_probe<M::value>; } };

extern "C" {

int jp_check_texture_mipmaps(const JpTextureMipmaps* m, int32_t* n_on)
{
	if (!m) return fail(JP_ERR_INVALID_ARGUMENT, "jp_check_texture_mipmaps: null argument");
	int a;
	const int st = check_texture_mipmaps(m, a);
	if (st == JP_OK && n_on) *n_on = a;
	return st;
}

int jp_set_texture_mipmaps(JpContext* c, const JpTextureMipmaps* m)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_texture_mipmaps: null context");
	if (!m) { c->mipmaps = MipmapsHost(); return JP_OK; }
	int a;
	if (const int st = check_texture_mipmaps(m, a); st != JP_OK) return st;
	MipmapsHost h;
	h.set = true; h.n_textures = m->n_textures; h.n_on = a; h.footprint_scale = m->footprint_scale; h.bounce_spread = m->bounce_spread;
	h.mode.assign((size_t)m->n_textures, JP_MIP_OFF);
	if (m->mode && m->n_textures > 0) h.mode.assign(m->mode, m->mode + m->n_textures);
	c->mipmaps = std::move(h);                                         // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_texture_mipmap_info(JpContext* c, JpTextureMipmapInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_mipmap_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_texture_mipmap_info: set JpTextureMipmapInfo.struct_bytes to sizeof(JpTextureMipmapInfo)");
	JpTextureMipmapInfo i; std::memset(&i, 0, sizeof(i));
	if (c->plan.have_scene && c->plan.mip_on > 0)
	{
		i.n_on = c->plan.mip_on; i.n_levels = c->plan.mip_levels; i.pyramid_bytes_device = c->plan.mip_bytes; i.build_ms = c->mip_build_ms;
		i.footprint_scale = c->plan.mv.footprint_scale; i.bounce_spread = c->plan.mv.bounce_spread; i.gamma0 = c->plan.mv.gamma0;
	}
	i.cone_bytes_device = (long long)c->cone.bytes();
	for (const JpContext* l : c->lanes) i.cone_bytes_device += (long long)l->cone.bytes();
	i.mip_last_render = c->last_mip;
	if (c->profiling && c->last_textured)
	{   // the side kernel's launches of the last render, all lanes (HIP-event times; synchronises)
		if (const int st = finish_counters(c); st != JP_OK) return st;
		i.texel_ms = c->texel_ms;
		for (int k = 1; k < c->last_lanes; k++) i.texel_ms += c->lanes[k - 1]->texel_ms;
	}
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_read_mip_chain(JpContext* c, int32_t texture, uint8_t* rgb8_out, int64_t capacity)
{
	if (!c || !rgb8_out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_mip_chain: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_read_mip_chain: no scene uploaded");
	if (c->plan.mip_on == 0 || texture < 0 || texture >= (int)c->mip_host_tex.size() || c->mip_host_tex[texture].y == 0)
		return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_mip_chain: texture " + std::to_string(texture) + " has no pyramid");
	const int2 ml = c->mip_host_tex[texture];
	long long total = 0;
	for (int k = 0; k < ml.y; k++) total += (long long)c->mip_host_lev[(size_t)ml.x + k].w * c->mip_host_lev[(size_t)ml.x + k].h;
	if (capacity < 3 * total) return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_mip_chain: capacity " + std::to_string(capacity) + " below the chain's " + std::to_string(3 * total) + " bytes");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	std::vector<unsigned int> tmp;
	size_t at = 0;
	for (int k = 0; k < ml.y; k++)
	{
		const JpMipLevel& l = c->mip_host_lev[(size_t)ml.x + k];
		const size_t n = (size_t)l.w * l.h;
		tmp.resize(n);
		HIP_TRY(hipMemcpy(tmp.data(), c->tab.texels.get<unsigned int>() + (size_t)l.first, n * 4, hipMemcpyDeviceToHost));
		unpack_rgb8(tmp.data(), n, rgb8_out + 3 * at);
		at += n;
	}
	return JP_OK;
}

int jp_build_mip_chain(int32_t w, int32_t h, const uint8_t* rgb8, uint8_t* rgb8_out, int32_t* level_w, int32_t* level_h, int32_t* n_levels)
{
	if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_mip_chain: size out of range (1 .. 16384 per side)");
	if (rgb8_out && !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_mip_chain: null argument");
	std::vector<JpMipLevel> lev;
	const long long total = mip_chain_layout(w, h, lev);
	if (n_levels) *n_levels = (int32_t)lev.size();
	for (size_t k = 0; k < lev.size(); k++) { if (level_w) level_w[k] = lev[k].w; if (level_h) level_h[k] = lev[k].h; }
	if (!rgb8_out) return JP_OK;
	std::vector<unsigned int> texels((size_t)total);
	pack_rgb8(rgb8, (size_t)w * h, texels.data());
	mip_chain_build(w, h, lev, texels);
	unpack_rgb8(texels.data(), texels.size(), rgb8_out);
	return JP_OK;
}

int jp_mip_cone_step(float gamma0, float bounce_spread, int32_t n, const int32_t* flags, const float* t, float* state)
{
	if (n < 0 || (n > 0 && (!flags || !t || !state))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_mip_cone_step: null argument");
	for (int32_t i = 0; i < n; i++) jp_mip_cone_hit(gamma0, bounce_spread, flags[i], t[i], state + 2 * (size_t)i, state + 2 * (size_t)i + 1);
	return JP_OK;
}

int jp_mip_footprint(int32_t n, const float* width, const float* area, int32_t w, int32_t h, float scale_u, float scale_v, float footprint_scale, float* rho_out)
{
	if (n < 0 || (n > 0 && (!width || !area || !rho_out))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_mip_footprint: null argument");
	for (int32_t i = 0; i < n; i++) rho_out[i] = jp_mip_rho(width[i], area[i], w, h, scale_u, scale_v, footprint_scale);
	return JP_OK;
}

int jp_texture_lookup_mip(const JpTexSampler* s, int32_t w, int32_t h, const uint8_t* rgb8, int32_t n, const float* uv, const float* rho, uint8_t* rgb8_out)
{
	if (n < 0 || (n > 0 && (!uv || !rho || !rgb8_out)) || !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_texture_lookup_mip: null argument");
	if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_texture_lookup_mip: size out of range (1 .. 16384 per side)");
	if (s) if (const int r = jp_tex_sampler_check(s, JP_TSAMP_COLOR)) return fail(JP_ERR_INVALID_ARGUMENT, std::string("jp_texture_lookup_mip: ") + jp_tex_sampler_rule(r));
	std::vector<JpMipLevel> lev;
	const long long total = mip_chain_layout(w, h, lev);
	std::vector<unsigned int> texels((size_t)total);
	pack_rgb8(rgb8, (size_t)w * h, texels.data());
	mip_chain_build(w, h, lev, texels);
	const bool active = s && !jp_tsamp_identity(s, JP_TSAMP_COLOR);
	const JpTexSampler id = jp_mip_identity_sampler();
	for (int32_t i = 0; i < n; i++)
	{
		const float u = uv[2 * (size_t)i], v = uv[2 * (size_t)i + 1], r = rho[i];
		unsigned int t;
		if (r > 1.f && r - r == 0.f) t = jp_mip_lookup_above(active ? s : &id, texels.data(), lev.data(), (int)lev.size(), u, v, r);
		else t = active ? jp_tex_lookup_sampled(s, texels.data(), w, h, u, v) : (texels[jp_tsamp_nearest_clamp(w, h, u, v)] & 0xffffffu);
		rgb8_out[3 * (size_t)i] = (uint8_t)(t & 0xffu); rgb8_out[3 * (size_t)i + 1] = (uint8_t)((t >> 8) & 0xffu); rgb8_out[3 * (size_t)i + 2] = (uint8_t)((t >> 16) & 0xffu);
	}
	return JP_OK;
}

int jp_mip_probe(JpContext* c, int32_t n, const float* origin, const float* dir, const float* tmin, const float* tmax, const int32_t* flags, float* state,
                 int32_t* prim, float* rho, uint8_t* rgb8)
{
	if (!c || n < 0 || !origin || !dir || !tmin || !tmax || !flags || !state || !prim || !rho || !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_mip_probe: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_mip_probe: no scene uploaded");
	if (c->plan.mip_on == 0) return fail(JP_ERR_UNSUPPORTED, "jp_mip_probe: the uploaded scene has no pyramid (jp_set_texture_mipmaps)");
	if (n == 0) return JP_OK;
	HIP_TRY(hipSetDevice(c->device));
	const TraceLaunch tk = trace_kernel(c->plan, 0);                // jp_surface's walk
	const MipProbeKernel pk = by_trace_mode(tk.mode & 15, MipProbeOf());
	if (!pk) return fail(JP_ERR_UNSUPPORTED, "jp_mip_probe: no instance for this walk");
	DevBuf b_in, b_out; float* d_in; float* d_out;                   // per-call scratch: freed on every return
	HIP_TRY(reserve(b_in, d_in, (size_t)n * 44)); HIP_TRY(reserve(b_out, d_out, (size_t)n * 12));
	float *d_o = d_in, *d_d = d_in + 3 * (size_t)n, *d_t0 = d_in + 6 * (size_t)n, *d_t1 = d_in + 7 * (size_t)n, *d_st = d_in + 8 * (size_t)n; int* d_fl = (int*)(d_in + 10 * (size_t)n);
	int* d_prim = (int*)d_out; float* d_rho = d_out + (size_t)n; unsigned int* d_w = (unsigned int*)(d_out + 2 * (size_t)n);
	HIP_TRY(hipMemcpyAsync(d_o, origin, (size_t)n * 12, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_d, dir, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_t0, tmin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_t1, tmax, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(d_st, state, (size_t)n * 8, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_fl, flags, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	const int grid = std::min(c->n_cus * 8, (n + JP_BLOCK - 1) / JP_BLOCK);
	hipLaunchKernelGGL(pk, dim3(grid), dim3(JP_BLOCK), tk.lds, c->stream, c->plan.sv, c->plan.tv, c->plan.sm, c->plan.mv, tk.depth, n, d_o, d_d, d_t0, d_t1, d_fl, d_st, d_prim, d_rho, d_w);
	HIP_TRY(hipGetLastError());
	std::vector<unsigned int> w((size_t)n);
	HIP_TRY(hipMemcpyAsync(prim, d_prim, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(rho, d_rho, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(state, d_st, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipMemcpyAsync(w.data(), d_w, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	for (int32_t i = 0; i < n; i++)
	{   // the colour the side word stands for, in bytes: an image's texel, or 0 for a colour of the table (solid / checker textures) and for no texture
		const unsigned int t = (w[i] & JP_TEX_IMAGE_TAG) ? w[i] : 0u;
		rgb8[3 * (size_t)i] = (uint8_t)(t & 0xffu); rgb8[3 * (size_t)i + 1] = (uint8_t)((t >> 8) & 0xffu); rgb8[3 * (size_t)i + 2] = (uint8_t)((t >> 16) & 0xffu);
	}
	return JP_OK;
}

} // extern "C"
#endif // JP_MIPMAP_RUNTIME
