// jet-pbrt_amd/csrc/jp_normal_map.h -- tangent-space normal maps (INTEGRATION.md "Normal maps", DESIGN.md "Normal maps"), in two parts like jp_normals.h:
//   part 1 (included before the kernels): NMapView and mapped_normal, the device side of include/jp_normal_map.h
//   part 2 (JP_NORMAL_MAP_RUNTIME, included before jp_normals.h's part 2, whose hook hands out k_shading_normal_mapped; launch_normal, jp_shade_launch.h, launches k_normal_map): k_normal_map, the test hook k_shading_normal_mapped, the upload's table step and the
//     entry points jp_set_normal_maps / jp_check_normal_maps / jp_get_normal_map_info / jp_perturb_normals / jp_triangle_tangents.
// A normal map is one more producer of the side record (Ns, 1) that k_shade_smooth* read: k_shade and the ten smooth families stay as they are.
// A context that never sets a normal map runs nothing of this file.
#ifndef JP_NORMAL_MAP_DEVICE_PART
#define JP_NORMAL_MAP_DEVICE_PART
#include "jp_common.h"
#include "jp_tex.h"
#include "jp_normals.h"
#include "../../include/jp_normal_map.h"
#include "jp_tex_sampling.h"      // part 1: SampView, SampSlot (texture sampling records: the map's addressing)

// ---- part 1 -----------------------------------------------------------------------------------------------------------------------------
// A separate kernel argument like NormView: the kernels of scenes without maps do not change.
struct NMapView
{
	const int4* desc;            // per map: (width, height, first texel in the pool, -)
	const unsigned int* texels;  // RGBA8 pool like TexView::texels: a tap is one load
	const float2* mat;           // per material: (map index as bits, -1 = none or a map that perturbs nothing; strength)
	const float2* prim_uv;       // three per primitive of the caller's order (JpNormalMaps.tri_uv); null: triangles stay unperturbed
};

namespace jp
{
// the geometric normal of a hit as k_shade forms it (k_trace's normal)
__device__ __forceinline__ V3 hit_normal(const float4* prims, int h, V3 p, V3 rd)
{
	const float4 g3 = prims[4 * h + 3]; const int type = __float_as_int(g3.w);
	if (type == JP_SHAPE_TRIANGLE) return xyz(g3);
	if (type == JP_SHAPE_RECTANGLE) return dot(xyz(g3), rd) <= 0 ? xyz(g3) : -xyz(g3);
	if (type == JP_SHAPE_DISK) return xyz(prims[4 * h + 1]);
	return normalize(p - xyz(prims[4 * h]));
}

// Ns' at the point p of device primitive h (caller's primitive index prim, material mat): N the geometric normal there, Nb the base normal (Ns of a smooth
// triangle, else N); false: unperturbed (Ns untouched).  slots (jp_tex_sampling.h; null: none): the maps' sampling records -- a map with an active one is addressed through it
__device__ __forceinline__ bool mapped_normal(const float4* prims, const NMapView& mp, int h, int prim, int mat, V3 p, V3 N, V3 Nb, V3& Ns, const SampSlot* slots = nullptr)
{
	if (mat < 0) return false;
	const float2 mm = mp.mat[mat];
	const int k = __float_as_int(mm.x);
	if (k < 0) return false;
	const float4 g0 = prims[4 * h], g3 = prims[4 * h + 3];
	const int type = __float_as_int(g3.w);
	float dpdu[3], dpdv[3];
	if (type == JP_SHAPE_TRIANGLE)
	{
		if (!mp.prim_uv) return false;
		const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
		const float2 t0 = mp.prim_uv[3 * prim], t1 = mp.prim_uv[3 * prim + 1], t2 = mp.prim_uv[3 * prim + 2];
		const float a0[3] = { g0.x, g0.y, g0.z }, a1[3] = { g1.x, g1.y, g1.z }, a2[3] = { g2.x, g2.y, g2.z }, uv6[6] = { t0.x, t0.y, t1.x, t1.y, t2.x, t2.y };
		if (!jp_triangle_tangents_at(a0, a1, a2, uv6, dpdu, dpdv)) return false;
	}
	else if (type == JP_SHAPE_RECTANGLE)
	{   // p3 rides in the w components (tex_uv)
		const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
		dpdu[0] = g1.x - g0.x; dpdu[1] = g1.y - g0.y; dpdu[2] = g1.z - g0.z;
		dpdv[0] = g0.w - g0.x; dpdv[1] = g1.w - g0.y; dpdv[2] = g2.w - g0.z;
	}
	else if (type == JP_SHAPE_DISK)
	{
		const Frame fr = frame_from_z(xyz(prims[4 * h + 1]));
		const V3 v0 = p - xyz(g0);
		const float s[3] = { fr.s.x, fr.s.y, fr.s.z }, t[3] = { fr.t.x, fr.t.y, fr.t.z }, v[3] = { v0.x, v0.y, v0.z };
		jp_disk_tangents_at(s, t, v, dpdu, dpdv);
	}
	else
	{
		const V3 d = p - xyz(g0);
		const float dd[3] = { d.x, d.y, d.z };
		jp_sphere_tangents_at(dd, dpdu, dpdv);
	}
	TexView tv = {}; tv.prim_uv = mp.prim_uv;
	const float2 uv = tex_uv(prims, tv, h, prim, p);
	const int4 md = mp.desc[k];
	const float nb[3] = { Nb.x, Nb.y, Nb.z }, ng[3] = { N.x, N.y, N.z };
	float ns[3];
	if (slots)
	{
		const SampSlot sl = slots[k];
		if (!jp_perturb_normal_sampled(sl.active ? &sl.s : nullptr, nb, ng, dpdu, dpdv, uv.x, uv.y, mp.texels + md.z, md.x, md.y, mm.y, ns)) return false;
	}
	else if (!jp_perturb_normal(nb, ng, dpdu, dpdv, uv.x, uv.y, mp.texels + md.z, md.x, md.y, mm.y, ns)) return false;
	Ns = mk(ns[0], ns[1], ns[2]);
	return true;
}

// the Ns the render uses at a hit of a mapped scene: the smooth triangle's Ns (nv.prim_vn may be null: no vertex normals), then the map on top; N where neither applies
__device__ __forceinline__ V3 mapped_shading_normal(const float4* prims, const NormView& nv, const NMapView& mp, int h, int prim, int mat, V3 p, V3 N, const SampSlot* slots = nullptr)
{
	V3 Nb = N;
	if (nv.prim_vn) shading_normal(prims, nv, h, prim, p, Nb);
	V3 Ns = Nb;
	mapped_normal(prims, mp, h, prim, mat, p, N, Nb, Ns, slots);
	return Ns;
}
} // namespace jp
#endif // JP_NORMAL_MAP_DEVICE_PART

#if defined(JP_NORMAL_MAP_RUNTIME) && !defined(JP_NORMAL_MAP_RUNTIME_PART)
#define JP_NORMAL_MAP_RUNTIME_PART
// ---- part 2: kernels ----------------------------------------------------------------------------------------------------------------------
// k_normal_map: k_normal's twin for a scene with at least one mapped material -- ONE kernel that does both jobs, because the map needs the smooth triangle's Ns as
// its base normal: a second kernel would read the record k_normal just wrote and gather hit -> primitive record -> meta again.  For every queued ray of the block's
// region: (Ns', 1) where the material's map perturbs the hit, (Ns, 1) on a smooth triangle it leaves alone, else 0 -- the record the position has without maps.
// A latency-bound dependent gather like k_texel and k_normal (hit -> primitive record -> meta -> material's map -> four texels), so it stays outside k_shade.
__global__ void __launch_bounds__(JP_BLOCK, 8) k_normal_map(SceneView sc, Queues q, int cur, NormView nv, NMapView mp)
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
					if (mapped_normal(sc.prims, mp, pi, meta.x, meta.y, p, N, on ? Ns : N, Ns)) on = true;
				}
				if (on) rec = make_float4(Ns.x, Ns.y, Ns.z, 1.f);
			}
		}
		nv.side[i] = rec;
	}
}

// k_shading_normal_mapped (jp_shading_normal on a mapped scene): k_shading_normal with the map on top -- an instance of its own, k_shading_normal keeps its code.
// sm.map (null: none): the maps' sampling records, a runtime branch -- the hook follows the records the render's k_normal_map_s follows
template <int kMode>
__global__ void __launch_bounds__(JP_BLOCK) k_shading_normal_mapped(SceneView sc, NormView nv, NMapView mp, SampView sm, int depth, int n, const float* o, const float* d, const float* tmin, const float* tmax_in,
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
			const int4 meta = sc.meta[h];
			const V3 p = ro + tmax * rd;
			pr = meta.x;
			N = hit_normal(sc.prims, h, p, rd);
			Ns = mapped_shading_normal(sc.prims, nv, mp, h, meta.x, meta.y, p, N, sm.map);
		}
		prim[i] = pr;
		ng[3 * i] = N.x; ng[3 * i + 1] = N.y; ng[3 * i + 2] = N.z;
		ns[3 * i] = Ns.x; ns[3 * i + 1] = Ns.y; ns[3 * i + 2] = Ns.z;
	}
}

namespace
{
typedef void (*ShadingNormalMappedKernel)(SceneView, NormView, NMapView, SampView, int, int, const float*, const float*, const float*, const float*, int*, float*, float*);
ShadingNormalMappedKernel shading_normal_mapped_kernel(const TraceLaunch& t) { return by_trace_mode(t.mode, [](auto m) -> ShadingNormalMappedKernel { return k_shading_normal_mapped<decltype(m)::value>; }); }

// everything of a JpNormalMaps that does not need the scene; n_mapped: materials with a map index >= 0
int check_normal_maps(const JpNormalMaps* m, long long& pool, int& n_mapped)
{
	pool = 0; n_mapped = 0;
	if (m->struct_bytes < (int32_t)sizeof(JpNormalMaps)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: set JpNormalMaps.struct_bytes to sizeof(JpNormalMaps)");
	if (m->n_maps < 0 || m->n_maps > (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: n_maps out of range");
	if (m->n_materials < 0 || m->n_triangles < 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: negative n_materials or n_triangles");
	if (m->n_maps > 0 && (!m->map_width || !m->map_height || !m->map_offset || !m->texels)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: null map_width / map_height / map_offset / texels");
	if (m->n_materials > 0 && !m->mat_map) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: null mat_map");
	for (int i = 0; i < m->n_maps; i++)
	{
		const long long w = m->map_width[i], h = m->map_height[i], off = m->map_offset[i];
		if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: map " + std::to_string(i) + ": size out of range (1 .. 16384 per side)");
		if (off < 0 || m->n_texel_bytes < 0 || off > m->n_texel_bytes - 3 * w * h) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: map " + std::to_string(i) + ": texels beyond n_texel_bytes");
		pool += w * h;
	}
	if (pool > 0x7fffffffll) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: more than 2^31 texels in all");
	for (int k = 0; k < m->n_materials; k++)
	{
		if (m->mat_map[k] < -1 || m->mat_map[k] >= m->n_maps) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: material " + std::to_string(k) + ": mat_map out of range");
		if (m->mat_strength && !std::isfinite(m->mat_strength[k])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: material " + std::to_string(k) + ": strength not finite");
		if (m->mat_map[k] >= 0) n_mapped++;
	}
	if (m->tri_uv) for (size_t k = 0; k < 6 * (size_t)m->n_triangles; k++) if (!std::isfinite(m->tri_uv[k])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: triangle " + std::to_string(k / 6) + ": uv not finite");
	return JP_OK;
}

float bits_as_float(int i) { float f; std::memcpy(&f, &i, sizeof(f)); return f; }   // (the host's __int_as_float)
// one dword per texel, as TexTables::texels
void pack_rgb8(const uint8_t* src, size_t n, unsigned int* dst)
{
	for (size_t k = 0; k < n; k++) dst[k] = (unsigned int)src[3 * k] | ((unsigned int)src[3 * k + 1] << 8) | ((unsigned int)src[3 * k + 2] << 16) | 0xff000000u;
}
}

// the upload's table step (jp_upload_scene with normal maps set; after upload_vertex_normals): the maps' descriptors and texel pool, the per-material and the
// per-primitive uv records, and the plan of a mapped scene -- the smooth row, like a scene with vertex normals
static int upload_normal_maps(JpContext* c, SceneTables& T, ScenePlan& plan, const JpScene* s)
{
	const NormalMapsHost& m = c->nmaps;
	if (m.n_materials != s->n_materials) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the normal maps' n_materials differs from the scene's (jp_set_normal_maps)");
	if (m.n_triangles != s->n_triangles) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: the normal maps' n_triangles differs from the scene's (jp_set_normal_maps)");
	// (what jp_get_normal_map_info reports rides in the plan: committed with it, so a refused upload leaves nothing behind)
	plan.nm_maps = (int)m.width.size(); plan.nm_mapped = m.n_mapped; plan.nm_texel_bytes = plan.nm_table_bytes = 0;
	// a map whose R and G are 128 everywhere decodes to mx = my = 0 at every tap: it perturbs nothing, like strength 0
	std::vector<float2> mat((size_t)std::max(1, s->n_materials), make_float2(bits_as_float(-1), 0.f));
	int effective = 0;
	for (int k = 0; k < s->n_materials; k++)
	{
		const int i = m.mat_map[k]; const float st = m.strength.empty() ? 1.f : m.strength[k];
		if (i < 0 || m.neutral[i] || st == 0.f) continue;
		mat[k] = make_float2(bits_as_float(i), st); effective++;
	}
	if (effective == 0) return JP_OK;                                   // nothing to perturb: the scene without maps, exactly
	std::vector<int4> desc(m.width.size());
	for (size_t i = 0; i < desc.size(); i++) desc[i] = make_int4(m.width[i], m.height[i], (int)m.first[i], 0);
	HIP_TRY(upload(T.nm_desc, desc.data(), desc.size() * sizeof(int4)));
	HIP_TRY(upload(T.nm_texels, m.texels.data(), m.texels.size() * sizeof(unsigned int)));
	HIP_TRY(upload(T.nm_mat, mat.data(), mat.size() * sizeof(float2)));
	NMapView mp = {}; mp.desc = T.nm_desc.get<int4>(); mp.texels = T.nm_texels.get<unsigned int>(); mp.mat = T.nm_mat.get<float2>();
	plan.nm_table_bytes = (long long)(desc.size() * sizeof(int4) + mat.size() * sizeof(float2));
	if (!m.tri_uv.empty() && s->n_primitives > 0)
	{
		std::vector<float2> puv(3 * (size_t)s->n_primitives, make_float2(0.f, 0.f));
		for (int p = 0; p < s->n_primitives; p++)
			if (s->prim_shape_type[p] == JP_SHAPE_TRIANGLE)
			{
				const float* u = m.tri_uv.data() + 6 * (size_t)s->prim_shape_index[p];
				for (int k = 0; k < 3; k++) puv[3 * (size_t)p + k] = make_float2(u[2 * k], u[2 * k + 1]);
			}
		HIP_TRY(upload(T.nm_prim_uv, puv.data(), puv.size() * sizeof(float2)));
		mp.prim_uv = T.nm_prim_uv.get<float2>();
		plan.nm_table_bytes += (long long)(puv.size() * sizeof(float2));
	}
	plan.nm_texel_bytes = (long long)(m.texels.size() * sizeof(unsigned int));
	plan.mp = mp; plan.mapped = true;
	if (!plan.smooth)
	{   // no smooth triangle: the smooth row all the same (upload_vertex_normals), with no vertex-normal table
		plan.nv = NormView(); plan.smooth = true;
		plan.tables_in_lds = false; plan.shade_prims_in_lds = false; plan.stage_nee = false; plan.shade_lds_bytes = 0;
	}
	return JP_OK;
}

extern "C" {

int jp_check_normal_maps(const JpNormalMaps* m, int32_t* n_mapped_materials)
{
	if (!m) return fail(JP_ERR_INVALID_ARGUMENT, "jp_check_normal_maps: null argument");
	long long pool; int nm;
	const int st = check_normal_maps(m, pool, nm);
	if (st == JP_OK && n_mapped_materials) *n_mapped_materials = nm;
	return st;
}

int jp_set_normal_maps(JpContext* c, const JpNormalMaps* m)
{
	if (!c) return fail(JP_ERR_INVALID_ARGUMENT, "jp_set_normal_maps: null context");
	if (!m) { c->nmaps = NormalMapsHost(); return JP_OK; }
	long long pool; int nm;
	if (const int st = check_normal_maps(m, pool, nm); st != JP_OK) return st;
	NormalMapsHost h; h.set = true; h.n_materials = m->n_materials; h.n_triangles = m->n_triangles; h.n_mapped = nm;
	h.texels.resize((size_t)pool);
	size_t at = 0;
	for (int i = 0; i < m->n_maps; i++)
	{
		const size_t n = (size_t)m->map_width[i] * (size_t)m->map_height[i];
		const uint8_t* src = m->texels + m->map_offset[i];
		h.width.push_back(m->map_width[i]); h.height.push_back(m->map_height[i]); h.first.push_back((long long)at);
		pack_rgb8(src, n, h.texels.data() + at);
		bool neutral = true;
		for (size_t k = 0; k < n && neutral; k++) neutral = src[3 * k] == 128 && src[3 * k + 1] == 128;
		h.neutral.push_back(neutral ? 1 : 0);
		at += n;
	}
	if (m->n_materials > 0) h.mat_map.assign(m->mat_map, m->mat_map + m->n_materials);
	if (m->mat_strength && m->n_materials > 0) h.strength.assign(m->mat_strength, m->mat_strength + m->n_materials);
	if (m->tri_uv && m->n_triangles > 0) h.tri_uv.assign(m->tri_uv, m->tri_uv + 6 * (size_t)m->n_triangles);
	c->nmaps = std::move(h);                                           // read by the next jp_upload_scene*
	return JP_OK;
}

int jp_get_normal_map_info(JpContext* c, JpNormalMapInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_normal_map_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_normal_map_info: set JpNormalMapInfo.struct_bytes to sizeof(JpNormalMapInfo)");
	JpNormalMapInfo i; std::memset(&i, 0, sizeof(i));
	if (c->plan.have_scene) { i.n_maps = c->plan.nm_maps; i.n_mapped_materials = c->plan.nm_mapped; i.texel_bytes_device = c->plan.nm_texel_bytes; i.table_bytes_device = c->plan.nm_table_bytes; }
	i.mapped_last_render = c->last_nmapped;
	if (c->profiling && c->last_nmapped)
	{   // k_normal_map's launches of the last render, all lanes (HIP-event times; synchronises)
		if (const int st = finish_counters(c); st != JP_OK) return st;
		i.normal_map_ms = c->normal_map_ms; for (int k = 1; k < c->last_lanes; k++) i.normal_map_ms += c->lanes[k - 1]->normal_map_ms;
	}
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}

int jp_perturb_normals(int32_t n, const float* nb, const float* ng, const float* dpdu, const float* dpdv, const float* uv,
                       int32_t width, int32_t height, const uint8_t* rgb8, float strength, float* ns_out, int32_t* perturbed_out)
{
	if (n < 0 || (n > 0 && (!nb || !ng || !dpdu || !dpdv || !uv || !ns_out || !perturbed_out)) || !rgb8) return fail(JP_ERR_INVALID_ARGUMENT, "jp_perturb_normals: null argument");
	if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_perturb_normals: size out of range (1 .. 16384 per side)");
	std::vector<unsigned int> texels((size_t)width * (size_t)height);
	pack_rgb8(rgb8, texels.size(), texels.data());
	for (int32_t i = 0; i < n; i++)
	{
		const size_t k = 3 * (size_t)i;
		float ns[3] = { nb[k], nb[k + 1], nb[k + 2] };                  // unperturbed: the base normal
		perturbed_out[i] = jp_perturb_normal(nb + k, ng + k, dpdu + k, dpdv + k, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], texels.data(), width, height, strength, ns);
		ns_out[k] = ns[0]; ns_out[k + 1] = ns[1]; ns_out[k + 2] = ns[2];
	}
	return JP_OK;
}

int jp_triangle_tangents(int32_t n, const float* p0, const float* p1, const float* p2, const float* uv6, float* dpdu, float* dpdv, int32_t* ok_out)
{
	if (n < 0 || (n > 0 && (!p0 || !p1 || !p2 || !uv6 || !dpdu || !dpdv || !ok_out))) return fail(JP_ERR_INVALID_ARGUMENT, "jp_triangle_tangents: null argument");
	for (int32_t i = 0; i < n; i++)
	{
		const size_t k = 3 * (size_t)i;
		float a[3] = { 0.f, 0.f, 0.f }, b[3] = { 0.f, 0.f, 0.f };
		ok_out[i] = jp_triangle_tangents_at(p0 + k, p1 + k, p2 + k, uv6 + 6 * (size_t)i, a, b);
		for (int j = 0; j < 3; j++) { dpdu[k + j] = a[j]; dpdv[k + j] = b[j]; }
	}
	return JP_OK;
}

} // extern "C"
#endif // JP_NORMAL_MAP_RUNTIME
