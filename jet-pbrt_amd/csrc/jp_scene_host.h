// jet-pbrt_amd/csrc/jp_scene_host.h -- host runtime, the upload's host half: check_scene (every index validated), the builders of the tables an upload hands to the
// device (HostTables: primitive records in leaf order, binary / 8-wide / 4-wide trees, the certified walk's tree over the caller's leaves, the flat leaf list,
// materials, lights, k_shade's LDS tables) and plan_scene (the ScenePlan every later launch reads).  Nothing here takes a JpContext or calls the HIP runtime:
// std::vector arithmetic on a JpScene, reachable without a device through jp_describe_upload (jp_upload.h) and tested in the CPU suite (tests/test_upload_host.py).
// Included by jp_kernels.hip after jp_runtime.h (fail, opt_flag, ScenePlan) and before jp_upload.h.
#pragma once
namespace
{
struct HV3 { float x, y, z; };
inline HV3 hsub(HV3 a, HV3 b) { HV3 r = { a.x - b.x, a.y - b.y, a.z - b.z }; return r; }
inline HV3 hcross(HV3 a, HV3 v) { HV3 r = { a.y * v.z - a.z * v.y, a.z * v.x - a.x * v.z, a.x * v.y - a.y * v.x }; return r; }
inline float hlen(HV3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline HV3 hld(const float* p) { HV3 r = { p[0], p[1], p[2] }; return r; }
inline HV3 hnorm(HV3 a) { const float l = hlen(a); HV3 r = { a.x / l, a.y / l, a.z / l }; return r; }
inline float box_area(const float* b) { float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2]; return dx * dy + dy * dz + dz * dx; }   // half the surface area
inline uint32_t pack4(const uint8_t* v) { return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24); }
inline uint64_t fnv1a(const void* p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } return h; }

// Binned-SAH binary tree over ITEM boxes with one item per leaf (certified walk: the items are the leaves of the caller's tree).
// left[n] >= 0: interior (left[n], right[n]); left[n] < 0: leaf holding item -left[n] - 1.  bounds: 6 floats per node.  Root = node 0.
struct ItemTree { std::vector<int> left, right; std::vector<float> bounds; int height = 0; };
int item_tree_build(const std::vector<float>& ib, std::vector<int>& idx, int start, int end, ItemTree& t, int depth)
{
	const int node = (int)t.left.size(); t.left.push_back(0); t.right.push_back(0); t.bounds.resize(t.bounds.size() + 6);
	t.height = std::max(t.height, depth);
	float nb[6] = { 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f }, cb[6] = { 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f };
	for (int i = start; i < end; i++)
	{
		const float* b = &ib[6 * (size_t)idx[i]];
		for (int a = 0; a < 3; a++) { nb[a] = std::min(nb[a], b[a]); nb[3 + a] = std::max(nb[3 + a], b[3 + a]); const float c = 0.5f * (b[a] + b[3 + a]); cb[a] = std::min(cb[a], c); cb[3 + a] = std::max(cb[3 + a], c); }
	}
	std::memcpy(&t.bounds[6 * (size_t)node], nb, sizeof(nb));
	if (end - start == 1) { t.left[node] = -idx[start] - 1; return node; }
	auto area = [](const float* b) { const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2]; return (dx < 0 || dy < 0 || dz < 0) ? 0.f : dx * dy + dy * dz + dz * dx; };   // (an empty bin run: 0, not box_area's product of negatives)
	const int NB = 16; float bestCost = 3.0e38f; int bestAxis = -1, bestBin = -1;
	for (int a = 0; a < 3; a++)
	{
		const float lo = cb[a], hi = cb[3 + a]; if (!(hi > lo)) continue;
		float bins[NB][6]; int cnt[NB];
		for (int k = 0; k < NB; k++) { for (int j = 0; j < 3; j++) { bins[k][j] = 1e30f; bins[k][3 + j] = -1e30f; } cnt[k] = 0; }
		const float scale = NB / (hi - lo);
		for (int i = start; i < end; i++)
		{
			const float* b = &ib[6 * (size_t)idx[i]];
			int k = (int)((0.5f * (b[a] + b[3 + a]) - lo) * scale); k = std::max(0, std::min(NB - 1, k));
			for (int j = 0; j < 3; j++) { bins[k][j] = std::min(bins[k][j], b[j]); bins[k][3 + j] = std::max(bins[k][3 + j], b[3 + j]); } cnt[k]++;
		}
		float rightArea[NB]; int rightCnt[NB]; float acc[6] = { 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f }; int c = 0;
		for (int k = NB - 1; k > 0; k--) { for (int j = 0; j < 3; j++) { acc[j] = std::min(acc[j], bins[k][j]); acc[3 + j] = std::max(acc[3 + j], bins[k][3 + j]); } c += cnt[k]; rightArea[k] = area(acc); rightCnt[k] = c; }
		for (int j = 0; j < 3; j++) { acc[j] = 1e30f; acc[3 + j] = -1e30f; } c = 0;
		for (int k = 0; k < NB - 1; k++)
		{
			for (int j = 0; j < 3; j++) { acc[j] = std::min(acc[j], bins[k][j]); acc[3 + j] = std::max(acc[3 + j], bins[k][3 + j]); } c += cnt[k];
			if (c == 0 || rightCnt[k + 1] == 0) continue;
			const float cost = area(acc) * c + rightArea[k + 1] * rightCnt[k + 1];
			if (cost < bestCost) { bestCost = cost; bestAxis = a; bestBin = k; }
		}
	}
	int mid = -1;
	if (bestAxis >= 0)
	{
		const int a = bestAxis; const float lo = cb[a], scale = NB / (cb[3 + a] - cb[a]);
		int* m = std::partition(idx.data() + start, idx.data() + end, [&](int i) { const float* b = &ib[6 * (size_t)i]; int k = (int)((0.5f * (b[a] + b[3 + a]) - lo) * scale); k = std::max(0, std::min(NB - 1, k)); return k <= bestBin; });
		mid = (int)(m - idx.data());
	}
	if (mid <= start || mid >= end)
	{   // coinciding centroids: split the range in the middle
		mid = start + (end - start) / 2;
	}
	const int l = item_tree_build(ib, idx, start, mid, t, depth + 1);
	const int r = item_tree_build(ib, idx, mid, end, t, depth + 1);
	t.left[node] = l; t.right[node] = r;
	return node;
}

int bvh_height(const JpScene* s, int node, int depth, int limit, bool& bad, std::vector<char>& seen)
{
	if (node < 0 || node >= s->n_bvh_nodes || seen[node] || depth > limit) { bad = true; return 0; }
	seen[node] = 1;
	if (s->bvh_left[node] < 0) return 0;                               // leaf
	int a = bvh_height(s, s->bvh_left[node], depth + 1, limit, bad, seen);
	int b = bvh_height(s, s->bvh_right[node], depth + 1, limit, bad, seen);
	return 1 + std::max(a, b);
}

// ---- validation: every index on the host, a bad index must never reach a kernel ----------------------------------------------------
// What the builders take over from the check: the nodes reachable from the root, the tree's height and leaf count, how the tree is to be used.
struct SceneCheck
{
	std::vector<char> seen; int height = 0, n_leaves = 0; bool has_null = false;
	bool device_build = false;                                         // no hierarchy handed over: build it on the device (jp_lbvh.h)
	bool ref_sem = false;                                              // walk the caller's tree with the reference's semantics (traverse_ref)
};
int check_scene(const JpScene* s, bool pick, SceneCheck& k)
{
	if (s->n_primitives <= 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: scene has no primitives");
	if (s->n_triangles < 0 || s->n_rectangles < 0 || s->n_spheres < 0 || s->n_disks < 0 || s->n_materials < 0 || s->n_lights < 0 || s->n_bvh_nodes < 0 || s->n_bvh_prim_indices < 0)
		return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: negative count");
	if (s->bvh_reference_semantics < 0 || s->bvh_reference_semantics > 2) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: bvh_reference_semantics must be 0, 1 or 2");
	if (s->bvh_reference_semantics != 0 && s->n_bvh_nodes == 0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: reference semantics need the caller's tree (n_bvh_nodes == 0)");
	const bool device_build = k.device_build = s->n_bvh_nodes == 0;
	k.ref_sem = !device_build && (s->bvh_reference_semantics == 1 || s->bvh_reference_semantics == 2);
	if (!s->prim_shape_type || !s->prim_shape_index || !s->prim_material || !s->prim_light || (!device_build && (!s->bvh_bounds || !s->bvh_left || !s->bvh_right || !s->bvh_prim_index)))
		return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: null array");
	if ((s->n_triangles && (!s->tri_p0 || !s->tri_p1 || !s->tri_p2 || !s->tri_n)) || (s->n_rectangles && (!s->rect_p0 || !s->rect_p1 || !s->rect_p2 || !s->rect_p3 || !s->rect_n))
	    || (s->n_spheres && (!s->sph_center || !s->sph_radius)) || (s->n_disks && (!s->disk_center || !s->disk_normal || !s->disk_radius)) || (s->n_materials && (!s->mat_type || !s->mat_params)) || (s->n_lights && (!s->light_type || !s->light_radiance || !s->light_prim)))
		return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: null array for a non-zero count");
	// pick: one light per bounce from the alias table (jp_pick.h), one shadow plane whatever the light count
	if (!pick && s->n_lights > 255) return fail(JP_ERR_UNSUPPORTED, "jp_upload_scene: more than 255 lights are not supported by the shadow-entry packing");
	if (pick && s->n_lights > (1 << 24)) return fail(JP_ERR_UNSUPPORTED, "jp_upload_scene: more than 2^24 lights (JP_LIGHTS_POWER_ONE)");
	for (int i = 0; i < s->n_primitives; i++)
	{
		int t = s->prim_shape_type[i], j = s->prim_shape_index[i];
		int lim = t == JP_SHAPE_TRIANGLE ? s->n_triangles : t == JP_SHAPE_RECTANGLE ? s->n_rectangles : t == JP_SHAPE_SPHERE ? s->n_spheres : t == JP_SHAPE_DISK ? s->n_disks : -1;
		if (lim < 0 || j < 0 || j >= lim) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: primitive shape reference out of range");
		if (s->prim_material[i] < -1 || s->prim_material[i] >= s->n_materials) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: primitive material out of range");
		if (s->prim_light[i] < -1 || s->prim_light[i] >= s->n_lights) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: primitive light out of range");
		if (s->prim_light[i] >= 0 && s->light_type[s->prim_light[i]] != JP_LIGHT_AREA) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: primitive light is not an area light");
		if (s->prim_material[i] < 0) k.has_null = true;
	}
	for (int i = 0; i < s->n_materials; i++) if (s->mat_type[i] < JP_MAT_MATTE || s->mat_type[i] > JP_MAT_METAL) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: unknown material type");
	for (int i = 0; i < s->n_lights; i++)
	{
		if (s->light_type[i] == JP_LIGHT_AREA) { if (s->light_prim[i] < 0 || s->light_prim[i] >= s->n_primitives) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: area light primitive out of range"); }
		else if (s->light_type[i] == JP_LIGHT_POINT || s->light_type[i] == JP_LIGHT_DIRECTION) { if (!s->light_vec) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: point / direction light without light_vec"); }
		else if (s->light_type[i] != JP_LIGHT_ENVIRONMENT) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: unknown light type");
	}
	// BVH: a tree, every primitive in exactly one leaf, leaf ranges in bounds, height within the LDS stack
	k.seen.assign(s->n_bvh_nodes, 0); bool bad = false;
	k.height = device_build ? 0 : bvh_height(s, 0, 0, 4 * JP_STACK_DEPTH, bad, k.seen);
	if (bad) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: BVH is not a tree rooted at node 0 (cycle, bad child index or excessive depth)");
	if (!device_build && k.height + 1 > JP_STACK_DEPTH) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: BVH height exceeds the device traversal stack (32)");
	std::vector<int> primSeen(s->n_primitives, 0);
	for (int n = 0; n < s->n_bvh_nodes; n++)
	{
		if (!k.seen[n] || s->bvh_left[n] >= 0) continue;
		k.n_leaves++;
		int first = -s->bvh_left[n] - 1, cnt = s->bvh_right[n];
		if (cnt < 1 || cnt > 16 || first < 0 || first + cnt > s->n_bvh_prim_indices) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: BVH leaf range invalid (1..16 primitives per leaf)");
		for (int j = 0; j < cnt; j++) { int p = s->bvh_prim_index[first + j]; if (p < 0 || p >= s->n_primitives) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: BVH primitive index out of range"); primSeen[p]++; }
	}
	if (!device_build) for (int i = 0; i < s->n_primitives; i++) if (primSeen[i] != 1) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: every primitive must be in exactly one BVH leaf");
	return JP_OK;
}
int check_leaf_encoding(const JpScene* s)
{
	return (size_t)s->n_primitives >= (1u << 27) ? fail(JP_ERR_UNSUPPORTED, "jp_upload_scene: too many primitives for the leaf reference encoding") : JP_OK;
}

// ---- the tables ------------------------------------------------------------------------------------------------------------------
enum { TAB_NODES, TAB_PRIMS, TAB_META, TAB_MATS, TAB_MAT_TYPE, TAB_LIGHTS, TAB_SHADE_TAB, TAB_WIDE, TAB_Q4, TAB_REFBOX, TAB_FLAT, TAB_COUNT };   // = JpUploadInfo::table, the order of the uploads
static_assert(TAB_COUNT == JP_UPLOAD_TABLES, "JpUploadInfo::table lists the host-built tables");
struct TableBytes { const void* data; size_t bytes; bool present; };  // present: this upload has the table on the host (an empty one still gets its 16 bytes on the device)

// What the size of a scene and the options select, for plan_scene: from HostTables::sizes(), or that with the device builders' results in it
struct PlanSizes { int n_nodes, n_prims, n_flat, height, wide_height, q4_height, planes; bool use_wide, use_q4, use_cert, has_null; };

// Everything an upload builds on the host: the vectors behind the device tables, and the scalars the plan and the views take from the builders
struct HostTables
{
	std::vector<float4> nodes, prims, refbox, flat, mats, lights, shade_tab; std::vector<int4> meta; std::vector<uint32_t> wide, q4; std::vector<int> mat_type;
	std::vector<int> devPrimOf;                                        // caller's primitive index -> device record
	std::vector<float> light_area;                                     // FShape::Area() per area light: the weights of the alias table (pick)
	bool device_build = false, use_wide = false, use_q4 = false, use_cert = false, has_null = false;
	int n_nodes = 0, n_wide = 0, n_q4 = 0;                             // node counts of the binary / 8-wide / 4-wide tables, whoever built them
	int height = 0, wide_height = 0, q4_height = 0, eye_leaves = 0, n_env = 0, planes = 0;
	float cert_pad = 0.f, cert_pad_eye = 0.f, env_sum[3] = { 0.f, 0.f, 0.f };
	PlanSizes sizes() const { PlanSizes z = { n_nodes, (int)meta.size(), (int)(flat.size() / 2), height, wide_height, q4_height, planes, use_wide, use_q4, use_cert, has_null }; return z; }
	void tables(TableBytes r[TAB_COUNT]) const                       // the bytes handed to upload(), table by table
	{
		auto some = [](const auto& v, bool on) { TableBytes b = { v.data(), on ? v.size() * sizeof(v[0]) : 0, on }; return b; };
		r[TAB_NODES] = some(nodes, !device_build); r[TAB_PRIMS] = some(prims, !device_build); r[TAB_META] = some(meta, !device_build);   // a device build moves its own into place
		r[TAB_MATS] = some(mats, true); r[TAB_MAT_TYPE] = some(mat_type, true); r[TAB_LIGHTS] = some(lights, true); r[TAB_SHADE_TAB] = some(shade_tab, true);
		r[TAB_WIDE] = some(wide, !wide.empty()); r[TAB_Q4] = some(q4, !q4.empty()); r[TAB_REFBOX] = some(refbox, !refbox.empty()); r[TAB_FLAT] = some(flat, !flat.empty());
	}
};

// Primitive records in the order the trees ask for them, and the boxes of the ordered walks.
// JpOptions::box_pad (diagnosis only, tools/gpu_fringe_census.py): every box of the host-built trees grows by this many scene units, so the walk
// also visits the leaves whose triangles accept a hit in the fp32 fringe OUTSIDE their exact box -- a stand-in for testing every primitive
struct RecordEmitter
{
	const JpScene* s; float extra_pad;
	std::vector<float4>& prims; std::vector<int4>& meta; std::vector<int>& devPrimOf;
	RecordEmitter(const JpScene* scene, const JpOptions& op, HostTables& t) : s(scene), extra_pad(std::max(0.f, op.box_pad)), prims(t.prims), meta(t.meta), devPrimOf(t.devPrimOf) { devPrimOf.assign(s->n_primitives, -1); }
	void padded_box(const float* src, float* b) const
	{
		for (int a = 0; a < 3; a++)
		{
			float lo = src[a], hi = src[3 + a];
			float m = std::max(std::fabs(lo), std::fabs(hi)); float e = m * 1e-6f + 1e-6f + extra_pad;   // >> ulp(m): flat (zero-extent) boxes stay hittable
			b[a] = lo - e; b[3 + a] = hi + e;
		}
	}
	void node_box(int n, float* b) const { padded_box(s->bvh_bounds + 6 * (size_t)n, b); }
	int emit_prim(int p)
	{
		const int dev = (int)meta.size(); devPrimOf[p] = dev;
		int t = s->prim_shape_type[p], i = s->prim_shape_index[p];
		float4 g[4] = { make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0) };
		if (t == JP_SHAPE_TRIANGLE)
		{
			g[0] = make_float4(s->tri_p0[3 * i], s->tri_p0[3 * i + 1], s->tri_p0[3 * i + 2], 0); g[1] = make_float4(s->tri_p1[3 * i], s->tri_p1[3 * i + 1], s->tri_p1[3 * i + 2], 0);
			g[2] = make_float4(s->tri_p2[3 * i], s->tri_p2[3 * i + 1], s->tri_p2[3 * i + 2], 0); g[3] = make_float4(s->tri_n[3 * i], s->tri_n[3 * i + 1], s->tri_n[3 * i + 2], 0);
		}
		else if (t == JP_SHAPE_RECTANGLE)
		{
			g[0] = make_float4(s->rect_p0[3 * i], s->rect_p0[3 * i + 1], s->rect_p0[3 * i + 2], s->rect_p3[3 * i]);
			g[1] = make_float4(s->rect_p1[3 * i], s->rect_p1[3 * i + 1], s->rect_p1[3 * i + 2], s->rect_p3[3 * i + 1]);
			g[2] = make_float4(s->rect_p2[3 * i], s->rect_p2[3 * i + 1], s->rect_p2[3 * i + 2], s->rect_p3[3 * i + 2]);
			g[3] = make_float4(s->rect_n[3 * i], s->rect_n[3 * i + 1], s->rect_n[3 * i + 2], 0);
		}
		else if (t == JP_SHAPE_DISK)
		{
			g[0] = make_float4(s->disk_center[3 * i], s->disk_center[3 * i + 1], s->disk_center[3 * i + 2], s->disk_radius[i]);
			g[1] = make_float4(s->disk_normal[3 * i], s->disk_normal[3 * i + 1], s->disk_normal[3 * i + 2], 0);
		}
		else g[0] = make_float4(s->sph_center[3 * i], s->sph_center[3 * i + 1], s->sph_center[3 * i + 2], s->sph_radius[i]);
		int tb = t; std::memcpy(&g[3].w, &tb, 4);
		for (int j = 0; j < 4; j++) prims.push_back(g[j]);
		int4 m; m.x = p; m.y = s->prim_material[p]; m.z = s->prim_light[p]; m.w = t; meta.push_back(m);
		return dev;
	}
	int emit_leaf(int n)                                             // the leaf reference of the binary and 4-wide trees
	{
		int first = -s->bvh_left[n] - 1, cnt = s->bvh_right[n];
		int dfirst = devPrimOf[s->bvh_prim_index[first]];                    // already placed by the wide-tree pass?
		if (dfirst < 0) { dfirst = (int)meta.size(); for (int k = 0; k < cnt; k++) emit_prim(s->bvh_prim_index[first + k]); }
		return -(((dfirst << 4) | (cnt - 1)) + 1);
	}
};

// ---- quantised child boxes (8-wide and 4-wide nodes): 8 bits per end on the grid lo + q * 2^e --------------------------------------
inline void quantise_scale(const float* lo, const float* hi, int eb[3], float sc3[3])
{
	for (int a = 0; a < 3; a++)
	{
		int e = (int)std::ceil(std::log2(std::max((hi[a] - lo[a]) / 255.f, 1e-30f)));
		e = std::max(-120, std::min(120, e));
		eb[a] = e + 127; sc3[a] = std::ldexp(1.0f, e);
	}
}
// one axis of a child box [blo, bhi]: rounded outwards, then walked outwards until it is conservative in fp32 as the device evaluates it.
// lo_ok / hi_ok: that end encloses the box (an end the 8 bits cannot reach does not); which of them is a failure is the caller's decision
struct QuantAxis { uint8_t q0, q1; bool lo_ok, hi_ok; };
inline QuantAxis quantise_box_axis(float blo, float bhi, float lo, float sc)
{
	int q0 = (int)std::floor((blo - lo) / sc), q1 = (int)std::ceil((bhi - lo) / sc);
	q0 = std::max(0, std::min(255, q0)); q1 = std::max(0, std::min(255, q1));
	while (q0 > 0 && std::fmaf((float)q0, sc, lo) > blo) q0--;
	while (q1 < 255 && std::fmaf((float)q1, sc, lo) < bhi) q1++;
	QuantAxis r = { (uint8_t)q0, (uint8_t)q1, !(std::fmaf((float)q0, sc, lo) > blo), !(std::fmaf((float)q1, sc, lo) < bhi) };
	return r;
}

// ---- large scenes: the binary tree collapsed into 8-wide nodes with quantised child boxes (traverse_wide) -------------------------
// Emits the primitives of every leaf it places (a leaf's records stay contiguous); false: a foreign BVH with leaves too large for the layout
bool build_wide8(RecordEmitter& em, std::vector<uint32_t>& wide, int& wide_height)
{
	const JpScene* s = em.s;
	struct Child { int node; int first, cnt, leaf_first, leaf_cnt; float b[6]; };   // node >= 0: inner (binary node index); else a chunk of <= 3 primitives of one binary leaf
	struct Item { int bnode; uint32_t widx; int depth; };
	std::vector<Item> queue; queue.push_back({ 0, 0u, 1 });
	wide.assign(20, 0u); wide_height = 0;
	std::vector<Child> ch; ch.reserve(16);                   // scratch reused across nodes (no allocation per wide node)
	queue.reserve((size_t)s->n_bvh_nodes / 2 + 16); wide.reserve(((size_t)s->n_bvh_nodes / 2 + 16) * 20);
	auto add = [&](int n) {
		float b[6]; em.node_box(n, b);
		if (s->bvh_left[n] >= 0) { Child c; c.node = n; c.first = c.cnt = c.leaf_first = c.leaf_cnt = 0; std::memcpy(c.b, b, sizeof(b)); ch.push_back(c); }
		else
		{
			int first = -s->bvh_left[n] - 1, cnt = s->bvh_right[n];
			for (int k = 0; k < cnt; k += 3) { Child c; c.node = -1; c.first = first + k; c.cnt = std::min(3, cnt - k); c.leaf_first = first; c.leaf_cnt = cnt; std::memcpy(c.b, b, sizeof(b)); ch.push_back(c); }
		}
	};
	auto slots_of = [&](int n) { return s->bvh_left[n] >= 0 ? 1 : (s->bvh_right[n] + 2) / 3; };
	for (size_t qi = 0; qi < queue.size(); qi++)
	{
		const Item it = queue[qi];
		wide_height = std::max(wide_height, it.depth);
		// gather up to 8 child slots: open the inner child with the largest box while the slots allow it
		ch.clear();
		add(s->bvh_left[it.bnode]); add(s->bvh_right[it.bnode]);
		for (;;)
		{
			int best = -1; float bestA = -1.f;
			for (size_t k = 0; k < ch.size(); k++)
				if (ch[k].node >= 0)
				{
					int need = (int)ch.size() - 1 + slots_of(s->bvh_left[ch[k].node]) + slots_of(s->bvh_right[ch[k].node]);
					if (need <= 8 && box_area(ch[k].b) > bestA) { bestA = box_area(ch[k].b); best = (int)k; }
				}
			if (best < 0) break;
			const int n = ch[best].node; ch.erase(ch.begin() + best);
			add(s->bvh_left[n]); add(s->bvh_right[n]);
		}
		if (ch.size() > 8) return false;
		// node box, scale exponents
		float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
		for (const Child& c : ch) for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], c.b[a]); hi[a] = std::max(hi[a], c.b[3 + a]); }
		int eb[3]; float sc3[3]; quantise_scale(lo, hi, eb, sc3);
		// slots: the three bits of a slot say on which side of the node centre the child lies (greedy assignment)
		int slotOf[8]; bool used[8] = { false, false, false, false, false, false, false, false };
		{
			struct Cand { float score; int child, slot; };
			Cand cands[64]; int ncand = 0;                     // <= 8 children x 8 slots, on the stack
			for (size_t k = 0; k < ch.size(); k++) for (int sl = 0; sl < 8; sl++)
			{
				float sc = 0;
				for (int a = 0; a < 3; a++) { float cc = 0.5f * (ch[k].b[a] + ch[k].b[3 + a]) - 0.5f * (lo[a] + hi[a]); sc += ((sl >> a) & 1) ? cc : -cc; }
				cands[ncand++] = { sc, (int)k, sl };
			}
			std::sort(cands, cands + ncand, [](const Cand& x, const Cand& y) { return x.score > y.score; });
			int got[8] = { -1, -1, -1, -1, -1, -1, -1, -1 };
			for (int ci = 0; ci < ncand; ci++) { const Cand& cd = cands[ci]; if (got[cd.child] < 0 && !used[cd.slot]) { got[cd.child] = cd.slot; used[cd.slot] = true; } }
			for (size_t k = 0; k < ch.size(); k++) slotOf[k] = got[k];
		}
		// emit: inner children get consecutive wide indices in slot order; leaf chunks append their primitives
		uint8_t metaB[8] = { 0 }, ql[3][8], qh[3][8]; uint32_t imask = 0;
		for (int sl = 0; sl < 8; sl++) for (int a = 0; a < 3; a++) { ql[a][sl] = 255; qh[a][sl] = 0; }
		const uint32_t child_base = (uint32_t)(wide.size() / 20);
		const uint32_t prim_base = (uint32_t)em.meta.size();
		int order[8], no = 0; for (int sl = 0; sl < 8; sl++) for (size_t k = 0; k < ch.size(); k++) if (slotOf[k] == sl) order[no++] = (int)k;
		uint32_t ninner = 0;
		for (int oi = 0; oi < no; oi++)
		{
			const Child& c = ch[order[oi]]; const int sl = slotOf[order[oi]];
			if (c.node >= 0) { imask |= 1u << sl; metaB[sl] = (uint8_t)(0x20 | (24 + sl)); queue.push_back({ c.node, child_base + ninner, it.depth + 1 }); ninner++; wide.resize(wide.size() + 20, 0u); }
			else
			{
				// the whole binary leaf is emitted when its first chunk comes up, so that its primitives stay contiguous on the
				// device and the binary tree (used for closest-hit rays) can address the same records
				if (em.devPrimOf[s->bvh_prim_index[c.first]] < 0) for (int k = 0; k < c.leaf_cnt; k++) em.emit_prim(s->bvh_prim_index[c.leaf_first + k]);
				const int poff = em.devPrimOf[s->bvh_prim_index[c.first]] - (int)prim_base;
				if (poff < 0 || poff + c.cnt > 24) return false;
				metaB[sl] = (uint8_t)((((1u << c.cnt) - 1u) << 5) | (unsigned)poff);
			}
			for (int a = 0; a < 3; a++)
			{
				const QuantAxis q = quantise_box_axis(c.b[a], c.b[3 + a], lo[a], sc3[a]);
				if (!q.hi_ok) return false;                           // (the lower end is the node's own: q = 0 reaches it)
				ql[a][sl] = q.q0; qh[a][sl] = q.q1;
			}
		}
		uint32_t* w = &wide[(size_t)it.widx * 20];
		std::memcpy(&w[0], &lo[0], 4); std::memcpy(&w[1], &lo[1], 4); std::memcpy(&w[2], &lo[2], 4);
		w[3] = (uint32_t)eb[0] | ((uint32_t)eb[1] << 8) | ((uint32_t)eb[2] << 16) | (imask << 24);
		w[4] = child_base; w[5] = prim_base; w[6] = pack4(metaB); w[7] = pack4(metaB + 4);
		w[8] = pack4(ql[0]); w[9] = pack4(ql[0] + 4); w[10] = pack4(ql[1]); w[11] = pack4(ql[1] + 4);
		w[12] = pack4(ql[2]); w[13] = pack4(ql[2] + 4); w[14] = pack4(qh[0]); w[15] = pack4(qh[0] + 4);
		w[16] = pack4(qh[1]); w[17] = pack4(qh[1] + 4); w[18] = pack4(qh[2]); w[19] = pack4(qh[2] + 4);
	}
	return true;
}

// ---- binary device tree (small and medium scenes; closest hits of large ones): children's boxes in the parent, interior nodes in DFS order
void build_binary(RecordEmitter& em, std::vector<float4>& nodes)
{
	const JpScene* s = em.s;
	const float kEmpty[6] = { 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f };
	if (s->bvh_left[0] < 0)
	{   // the root itself is a leaf: a synthetic interior root whose right child can never be hit
		float lb[6]; em.node_box(0, lb);
		int ref = em.emit_leaf(0), rr = ref; float fr, fl; std::memcpy(&fl, &ref, 4); std::memcpy(&fr, &rr, 4);
		nodes.push_back(make_float4(lb[0], lb[1], lb[2], lb[3])); nodes.push_back(make_float4(lb[4], lb[5], kEmpty[0], kEmpty[1]));
		nodes.push_back(make_float4(kEmpty[2], kEmpty[3], kEmpty[4], kEmpty[5])); nodes.push_back(make_float4(fl, fr, 0, 0));
		return;
	}
	std::vector<int> order, hostToDevNode(s->n_bvh_nodes, -1), st; st.push_back(0);
	while (!st.empty()) { int n = st.back(); st.pop_back(); if (s->bvh_left[n] < 0) continue; hostToDevNode[n] = (int)order.size(); order.push_back(n); st.push_back(s->bvh_right[n]); st.push_back(s->bvh_left[n]); }
	nodes.resize(4 * order.size());
	for (size_t di = 0; di < order.size(); di++)
	{
		int n = order[di], l = s->bvh_left[n], r = s->bvh_right[n];
		float lb[6], rb[6]; em.node_box(l, lb); em.node_box(r, rb);
		int lref = s->bvh_left[l] < 0 ? em.emit_leaf(l) : hostToDevNode[l];
		int rref = s->bvh_left[r] < 0 ? em.emit_leaf(r) : hostToDevNode[r];
		float fl, fr; std::memcpy(&fl, &lref, 4); std::memcpy(&fr, &rref, 4);
		nodes[4 * di + 0] = make_float4(lb[0], lb[1], lb[2], lb[3]); nodes[4 * di + 1] = make_float4(lb[4], lb[5], rb[0], rb[1]);
		nodes[4 * di + 2] = make_float4(rb[2], rb[3], rb[4], rb[5]); nodes[4 * di + 3] = make_float4(fl, fr, 0, 0);
	}
}

// ---- reference semantics: the caller's nodes under their own indices, unpadded boxes; primitives in the leaves' visiting order (left before right)
struct LeafItems { std::vector<int> first, cnt; std::vector<float> box; };   // the leaves of the caller's tree: device primitive range, exact box
void build_reference_nodes(RecordEmitter& em, std::vector<float4>& nodes, LeafItems& leaves)
{
	const JpScene* s = em.s;
	nodes.assign((size_t)2 * s->n_bvh_nodes, make_float4(0, 0, 0, 0));
	std::vector<int> st; st.push_back(0);
	while (!st.empty())
	{
		const int n = st.back(); st.pop_back();
		const float* b = s->bvh_bounds + 6 * (size_t)n;
		int l = s->bvh_left[n], r = s->bvh_right[n];
		if (l < 0)
		{
			const int first = -l - 1, cnt = r;
			const int dfirst = (int)em.meta.size();
			for (int k = 0; k < cnt; k++) em.emit_prim(s->bvh_prim_index[first + k]);
			l = -dfirst - 1;
			leaves.first.push_back(dfirst); leaves.cnt.push_back(cnt); leaves.box.insert(leaves.box.end(), b, b + 6);
		}
		else { st.push_back(r); st.push_back(l); }
		float fl, fr; std::memcpy(&fl, &l, 4); std::memcpy(&fr, &r, 4);
		nodes[2 * (size_t)n] = make_float4(b[0], b[1], b[2], fl); nodes[2 * (size_t)n + 1] = make_float4(b[3], b[4], b[5], fr);
	}
}

// ---- large scenes: a binary tree collapsed into 4-wide nodes with quantised child boxes (Walker<4>, Walker<6>) -----------------------
// From binary node b: its two children, then the interior child with the largest box is opened again while fewer than four
// slots are taken.  Leaves keep the binary tree's encoding and primitive records.  One collapse for two sources: the caller's tree as it
// is, and -- reference semantics, certified walk -- the tree built over the caller's leaves.
template <class IsInner, class LeftOf, class RightOf, class BoxOf, class LeafRefOf, class FlagOf>
bool collapse_q4(size_t n_nodes, IsInner isInner, LeftOf leftOf, RightOf rightOf, BoxOf boxOf, LeafRefOf leafRefOf, FlagOf flagOf, std::vector<uint32_t>& q4, int& q4_height)
{
	struct Item { int bnode; uint32_t idx; int depth; };
	std::vector<Item> queue; queue.reserve(n_nodes / 2 + 16); queue.push_back({ 0, 0u, 1 });
	q4.clear(); q4_height = 0; q4.reserve((n_nodes / 2 + 16) * 16); q4.assign(16, 0u);
	for (size_t qi = 0; qi < queue.size(); qi++)
	{
		const Item it = queue[qi];
		q4_height = std::max(q4_height, it.depth);
		int ch[4]; float cb[4][6]; int nc = 0;
		ch[nc] = leftOf(it.bnode); boxOf(ch[nc], cb[nc]); nc++;
		ch[nc] = rightOf(it.bnode); boxOf(ch[nc], cb[nc]); nc++;
		while (nc < 4)
		{
			int best = -1; float bestA = -1.f;
			for (int k = 0; k < nc; k++) if (isInner(ch[k]) && box_area(cb[k]) > bestA) { bestA = box_area(cb[k]); best = k; }
			if (best < 0) break;
			const int n = ch[best];
			ch[best] = leftOf(n); boxOf(ch[best], cb[best]);
			ch[nc] = rightOf(n); boxOf(ch[nc], cb[nc]); nc++;
		}
		float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
		for (int k = 0; k < nc; k++) for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], cb[k][a]); hi[a] = std::max(hi[a], cb[k][3 + a]); }
		// Walker<4> evaluates a slab distance as q * (2^e / d) + (p - o) / d: its rounding error grows with the NODE's extent, so every
		// child box gets 1e-6 of the node's extent on top of the relative padding of the box source before it is quantised outward
		for (int k = 0; k < nc; k++) for (int a = 0; a < 3; a++) { const float ex = 1e-6f * (hi[a] - lo[a]); cb[k][a] -= ex; cb[k][3 + a] += ex; }
		for (int a = 0; a < 3; a++) { const float ex = 1e-6f * (hi[a] - lo[a]); lo[a] -= ex; hi[a] += ex; }
		int eb[3]; float sc3[3]; quantise_scale(lo, hi, eb, sc3);
		uint8_t ql[3][4], qh[3][4]; uint32_t refs[4] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu }, valid = 0, flags = 0;   // unused slots: the empty box (255 > 0) and primitive 0 as a one-primitive leaf (-1): WalkerQ4 tests no valid bit
		for (int k = 0; k < 4; k++) for (int a = 0; a < 3; a++) { ql[a][k] = 255; qh[a][k] = 0; }
		for (int k = 0; k < nc; k++)
		{
			valid |= 1u << k;
			const int n = ch[k];
			if (flagOf(n)) flags |= 1u << k;
			int r;
			if (isInner(n)) { r = (int)(q4.size() / 16); queue.push_back({ n, (uint32_t)r, it.depth + 1 }); q4.resize(q4.size() + 16, 0u); }
			else r = leafRefOf(n);
			std::memcpy(&refs[k], &r, 4);
			for (int a = 0; a < 3; a++)
			{
				const QuantAxis q = quantise_box_axis(cb[k][a], cb[k][3 + a], lo[a], sc3[a]);
				if (!q.hi_ok || !q.lo_ok) return false;               // (the node's box was widened after the children's: both ends can miss)
				ql[a][k] = q.q0; qh[a][k] = q.q1;
			}
		}
		uint32_t* w = &q4[(size_t)it.idx * 16];
		std::memcpy(&w[0], &lo[0], 4); std::memcpy(&w[1], &lo[1], 4); std::memcpy(&w[2], &lo[2], 4);
		w[3] = (uint32_t)eb[0] | ((uint32_t)eb[1] << 8) | ((uint32_t)eb[2] << 16) | (valid << 24);
		w[4] = refs[0]; w[5] = refs[1]; w[6] = refs[2]; w[7] = refs[3];
		w[8] = pack4(ql[0]); w[9] = pack4(ql[1]); w[10] = pack4(ql[2]); w[11] = pack4(qh[0]);
		w[12] = pack4(qh[1]); w[13] = pack4(qh[2]); w[14] = flags; w[15] = 0;
	}
	return true;
}
// the caller's tree for the closest-hit rays (JpOptions::q4 = -1: they walk the binary tree)
bool build_q4(RecordEmitter& em, std::vector<uint32_t>& q4, int& q4_height)
{
	const JpScene* s = em.s;
	return collapse_q4((size_t)s->n_bvh_nodes, [s](int n) { return s->bvh_left[n] >= 0; }, [s](int n) { return s->bvh_left[n]; }, [s](int n) { return s->bvh_right[n]; },
	                   [&em](int n, float* bb) { em.node_box(n, bb); }, [&em](int n) { return em.emit_leaf(n); }, [](int) { return false; }, q4, q4_height);
}

// ---- reference semantics on large scenes: the certified walk (Walker<6>, jp_device.h) ----------------------------------------------
// A binned-SAH tree over the LEAVES of the caller's tree (their exact boxes, padded like every box of the ordered walks), collapsed to 4-wide
// nodes; a leaf of it is one leaf of the caller's tree (same primitive range, same order).  Per primitive the exact box of its leaf
// (the certificate is FBounds3::Intersect on that box).  The caller's nodes stay on the device for the rays that get no certificate.
// false: the verbatim walk serves (t.q4 left empty)
bool build_certified(const RecordEmitter& em, const JpOptions& op, const LeafItems& lv, HostTables& t)
{
	const JpScene* s = em.s;
	const int ni = (int)lv.first.size();
	ItemTree it; std::vector<int> idx(ni); for (int i = 0; i < ni; i++) idx[i] = i;
	it.left.reserve(2 * (size_t)ni); it.right.reserve(2 * (size_t)ni); it.bounds.reserve(12 * (size_t)ni);
	item_tree_build(lv.box, idx, 0, ni, it, 1);
	bool ok = it.left[0] >= 0 && it.height + 2 <= 48;
	for (int i = 0; i < ni && ok; i++) if (lv.cnt[i] < 1 || lv.cnt[i] > 16) ok = false;
	// "edge-on to the camera": a leaf holding a flat primitive whose plane passes the eye within tau of its distance -- the only primitives a CAMERA ray can
	// lie in to within fp32 noise, i.e. whose acceptance far in front of their leaf's box an ordered walk would cull (Walker<6>).  Flag = leaf, and every node above it.
	const float tau = op.cert_eye_tau == 0.f ? 5e-3f : std::max(0.f, op.cert_eye_tau);
	std::vector<char> item_eye(ni, 0), node_eye(it.left.size(), 0); t.eye_leaves = 0;
	for (int i = 0; i < ni && ok; i++)
		for (int k = 0; k < lv.cnt[i]; k++)
		{
			const size_t p = (size_t)lv.first[i] + k;
			int type; std::memcpy(&type, &t.prims[4 * p + 3].w, 4);
			if (type == JP_SHAPE_SPHERE) continue;
			const float4 g0 = t.prims[4 * p], gn = type == JP_SHAPE_DISK ? t.prims[4 * p + 1] : t.prims[4 * p + 3];
			const double vx = (double)g0.x - s->camera.pos[0], vy = (double)g0.y - s->camera.pos[1], vz = (double)g0.z - s->camera.pos[2];
			const double nl = std::sqrt((double)gn.x * gn.x + (double)gn.y * gn.y + (double)gn.z * gn.z), dist = std::sqrt(vx * vx + vy * vy + vz * vz);
			if (std::fabs(vx * gn.x + vy * gn.y + vz * gn.z) <= tau * dist * nl + 1e-30) { if (!item_eye[i]) t.eye_leaves++; item_eye[i] = 1; }
		}
	if (ok) for (size_t n = it.left.size(); n-- > 0;) node_eye[n] = it.left[n] < 0 ? item_eye[-it.left[n] - 1] : (char)(node_eye[it.left[n]] | node_eye[it.right[n]]);   // children have higher indices than their parent
	if (ok) ok = collapse_q4(it.left.size(), [&it](int n) { return it.left[n] >= 0; }, [&it](int n) { return it.left[n]; }, [&it](int n) { return it.right[n]; },
	                         [&](int n, float* bb) { em.padded_box(&it.bounds[6 * (size_t)n], bb); },
	                         [&](int n) { const int item = -it.left[n] - 1; return -(((lv.first[item] << 4) | (lv.cnt[item] - 1)) + 1); }, [&](int n) { return node_eye[n] != 0; }, t.q4, t.q4_height);
	if (!ok) { t.q4.clear(); return false; }
	t.refbox.resize((size_t)2 * s->n_primitives);
	double diag = 0;
	for (int i = 0; i < ni; i++)
	{
		const float* b = &lv.box[6 * (size_t)i];
		for (int k = 0; k < lv.cnt[i]; k++) { const size_t p = (size_t)lv.first[i] + k; t.refbox[2 * p] = make_float4(b[0], b[1], b[2], 0.f); t.refbox[2 * p + 1] = make_float4(b[3], b[4], b[5], 0.f); }
		diag += std::sqrt((double)(b[3] - b[0]) * (b[3] - b[0]) + (double)(b[4] - b[1]) * (b[4] - b[1]) + (double)(b[5] - b[2]) * (b[5] - b[2]));
	}
	// distance-cull slack: a hit in the fp32 acceptance fringe of FTriangle::Intersect lies up to ~ eps * D^2 / edge beside its triangle (D: distance
	// from the ray origin), so up to a few times that in front of its leaf's box -- with a 1 / distance tail for rays grazing the box: tmax + K * eps / (mean leaf
	// diagonal) * tmax^2.  K = 1024: 3 of 259,200 pixels of the configs[4] shard (3.1e9 rays) off; 16384: none, for 4 % of the frame rate (profiles/r03l_certified_walk.txt)
	const float K = op.cert_slack == 0.f ? 16384.f : std::max(0.f, op.cert_slack);
	t.cert_pad = (float)(K * 1.1920929e-7 / std::max(1e-20, diag / ni));
	// rays from the camera position: their noise planes are covered by the edge-on flags, so the slack only has to cover the fringe in front of a leaf's box
	const float Ke = op.cert_slack_eye == 0.f ? std::min(K, 1024.f) : std::max(0.f, op.cert_slack_eye);
	t.cert_pad_eye = (float)(Ke * 1.1920929e-7 / std::max(1e-20, diag / ni));
	return true;
}

// ---- tiny scenes: the flat leaf list of flat_boxes (leaf boxes padded like the node boxes, each with the bit set of its primitives) --
void build_flat(const RecordEmitter& em, const SceneCheck& k, std::vector<float4>& flat)
{
	const JpScene* s = em.s;
	if (s->n_primitives > 64 || k.n_leaves > 32) return;
	for (int n = 0; n < s->n_bvh_nodes; n++)
	{
		if (!k.seen[n] || s->bvh_left[n] >= 0) continue;
		float bb[6]; em.node_box(n, bb);
		int first = -s->bvh_left[n] - 1, cnt = s->bvh_right[n];
		unsigned long long bits = 0;
		for (int j = 0; j < cnt; j++) bits |= 1ull << em.devPrimOf[s->bvh_prim_index[first + j]];
		const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32); float flo, fhi; std::memcpy(&flo, &lo, 4); std::memcpy(&fhi, &hi, 4);
		flat.push_back(make_float4(bb[0], bb[1], bb[2], flo)); flat.push_back(make_float4(bb[3], bb[4], bb[5], fhi));
	}
}

// ---- materials: the 16-float rows as 4 x float4; lights: (radiance, type) (device prim, 1/Area(), -, -) -------------------------------
// areas with the reference's expressions (shape.h:351, 457, 546); needs devPrimOf, so it runs after the trees (or the device build)
void build_material_light_tables(const JpScene* s, bool pick, HostTables& t)
{
	t.mats.assign(4 * (size_t)std::max(1, s->n_materials), make_float4(0, 0, 0, 0)); t.mat_type.assign(std::max(1, s->n_materials), 0);
	for (int i = 0; i < s->n_materials; i++) { std::memcpy(&t.mats[4 * i], s->mat_params + (size_t)i * JP_MAT_PARAM_STRIDE, 16 * sizeof(float)); t.mat_type[i] = s->mat_type[i]; }
	t.lights.assign(2 * (size_t)std::max(1, s->n_lights), make_float4(0, 0, 0, 0)); t.planes = t.n_env = 0; t.env_sum[0] = t.env_sum[1] = t.env_sum[2] = 0.f;
	t.light_area.assign(pick ? (size_t)s->n_lights : 0, 0.f);
	for (int i = 0; i < s->n_lights; i++)
	{
		int ty = s->light_type[i]; float tf; std::memcpy(&tf, &ty, 4);
		const float* rad = s->light_radiance + 3 * i;
		t.lights[2 * i] = make_float4(rad[0], rad[1], rad[2], tf);
		bool black = rad[0] == 0.f && rad[1] == 0.f && rad[2] == 0.f;
		if (!black) t.planes++;
		float inv_area = 0.f; int dp = -1;
		if (ty == JP_LIGHT_AREA)
		{
			int p = s->light_prim[i]; dp = t.devPrimOf[p];
			int st = s->prim_shape_type[p], k = s->prim_shape_index[p]; float area;
			if (st == JP_SHAPE_TRIANGLE) area = 0.5f * hlen(hcross(hsub(hld(s->tri_p1 + 3 * k), hld(s->tri_p0 + 3 * k)), hsub(hld(s->tri_p2 + 3 * k), hld(s->tri_p0 + 3 * k))));
			else if (st == JP_SHAPE_RECTANGLE) area = hlen(hcross(hsub(hld(s->rect_p0 + 3 * k), hld(s->rect_p1 + 3 * k)), hsub(hld(s->rect_p2 + 3 * k), hld(s->rect_p1 + 3 * k))));
			else if (st == JP_SHAPE_DISK) { const float kPi = (float)3.14159265358979323846; area = kPi * s->disk_radius[k] * s->disk_radius[k]; }   // shape.h:253
			else { const float kPi = (float)3.14159265358979323846; float r2 = s->sph_radius[k] * s->sph_radius[k]; area = 4 * kPi * r2; }
			inv_area = 1 / area;
			if (pick) t.light_area[i] = area;
		}
		else if (ty == JP_LIGHT_ENVIRONMENT) { t.n_env++; t.env_sum[0] += rad[0]; t.env_sum[1] += rad[1]; t.env_sum[2] += rad[2]; }
		float df; std::memcpy(&df, &dp, 4);
		t.lights[2 * i + 1] = make_float4(df, inv_area, 0, 0);
		if (ty == JP_LIGHT_POINT || ty == JP_LIGHT_DIRECTION) t.lights[2 * i + 1] = make_float4(s->light_vec[3 * i], s->light_vec[3 * i + 1], s->light_vec[3 * i + 2], 0);
	}
}

// ---- k_shade's LDS tables as one array (SceneView::shade_tab); the primitive part only when the host has the records in device order --
void build_shade_tab(const JpScene* s, bool pick, HostTables& t)
{
	std::vector<float4>& tabv = t.shade_tab; tabv.clear();
	if (!pick) tabv.insert(tabv.end(), t.lights.begin(), t.lights.begin() + 2 * (size_t)s->n_lights);          // exactly the counts the kernel indexes with (the pick kernels: no light records)
	tabv.insert(tabv.end(), t.mats.begin(), t.mats.begin() + 4 * (size_t)s->n_materials);
	const size_t at = tabv.size(); tabv.resize(at + ((size_t)s->n_materials + 3) / 4, make_float4(0, 0, 0, 0));
	if (s->n_materials > 0) std::memcpy(&tabv[at], t.mat_type.data(), (size_t)s->n_materials * sizeof(int));
	if (t.device_build) return;
	tabv.insert(tabv.end(), t.prims.begin(), t.prims.end());
	const size_t am = tabv.size(); tabv.resize(am + t.meta.size());
	std::memcpy(&tabv[am], t.meta.data(), t.meta.size() * sizeof(int4));
	// FFrame(normal) (geometry.h:345-349, 371-376) of every flat primitive's stored normal, operation by operation as
	// frame_from_z does it on the device (this file is compiled with -ffp-contract=off for the host too)
	for (size_t pi = 0; pi < t.meta.size(); pi++)
	{
		const float4 g3 = t.prims[4 * pi + 3], g1 = t.prims[4 * pi + 1];
		int type; std::memcpy(&type, &g3.w, 4);
		const HV3 nn = type == JP_SHAPE_DISK ? HV3{ g1.x, g1.y, g1.z } : HV3{ g3.x, g3.y, g3.z };
		const HV3 n = hnorm(nn);
		const HV3 tmp = std::fabs(n.x) > 0.99f ? HV3{ 0, 1, 0 } : HV3{ 1, 0, 0 };
		const HV3 tg = hnorm(hcross(n, tmp)), sv = hnorm(hcross(tg, n));
		tabv.push_back(make_float4(n.x, n.y, n.z, 0)); tabv.push_back(make_float4(sv.x, sv.y, sv.z, 0)); tabv.push_back(make_float4(tg.x, tg.y, tg.z, 0));
	}
}

// ---- every table of a host-built hierarchy, in the order that fixes the device primitive order: the 8-wide pass first, then the binary
// and 4-wide trees, which find those records through devPrimOf ---------------------------------------------------------------------
int build_host_tables(const JpScene* s, const JpOptions& op, bool pick, const SceneCheck& k, HostTables& t)
{
	if (const int st = check_leaf_encoding(s); st != JP_OK) return st;
	RecordEmitter em(s, op, t);
	t.height = k.height; t.has_null = k.has_null;
	const bool inner_root = s->bvh_left[0] >= 0;
	if (k.ref_sem)
	{
		LeafItems leaves;
		build_reference_nodes(em, t.nodes, leaves);
		// (JpOptions::certified = -1 downgrades to the verbatim walk; nothing upgrades a scene that asked for it)
		const bool want_cert = s->bvh_reference_semantics == 2 && op.certified >= 0 && s->n_primitives > 1024 && leaves.first.size() >= 64;
		t.use_cert = want_cert && build_certified(em, op, leaves, t);
	}
	else
	{
		t.use_wide = k.n_leaves > 32 && inner_root;
		if (((size_t)s->n_bvh_nodes + (size_t)s->n_primitives) * 80 + (size_t)(k.height + 2) * JP_BLOCK * sizeof(int) <= 40 * 1024) t.use_wide = false;   // LDS-resident scenes keep the binary tree
		if (op.traversal > 0) { const int m = op.traversal - 1; if (m == 3 && inner_root) t.use_wide = true; else if (m >= 0 && m <= 2) t.use_wide = false; }
		if (t.use_wide && (!build_wide8(em, t.wide, t.wide_height) || (int)t.meta.size() != s->n_primitives))
		{   // a foreign BVH with leaves too large for the wide layout: keep the binary tree
			t.use_wide = false; t.wide.clear(); t.prims.clear(); t.meta.clear(); std::fill(t.devPrimOf.begin(), t.devPrimOf.end(), -1);
		}
		build_binary(em, t.nodes);
		t.use_q4 = s->n_primitives > 1024 && inner_root && opt_flag(op.q4, true);
		if (t.use_q4 && (!build_q4(em, t.q4, t.q4_height) || (int)t.meta.size() != s->n_primitives)) { t.use_q4 = false; t.q4.clear(); }
		build_flat(em, k, t.flat);
	}
	t.n_nodes = (int)(t.nodes.size() / 4); t.n_wide = (int)(t.wide.size() / 20); t.n_q4 = (int)(t.q4.size() / 16);
	build_material_light_tables(s, pick, t);
	build_shade_tab(s, pick, t);
	return JP_OK;
}

// ---- the alias table of JP_LIGHTS_POWER_ONE (jp_pick.h) and of the environment map's texels (jp_env.h) ----------------------------------
// Vose's alias method in double.  Bins of weight 0 are paired first, while the bins above average still hold all of their excess, so rounding
// can never leave one of them to the closing "threshold 1" step: a light of weight 0 is in no bin's reach.  W: the weights summed in index order.
int build_light_table(int n, const double* w, float* q, int32_t* alias, float* pmf, double* W_out, int* n_sel_out)
{
	double W = 0.0; int nsel = 0;
	for (int i = 0; i < n; i++)
	{
		if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_light_table: a weight is negative or not finite");
		W += w[i]; if (w[i] > 0.0) nsel++;
	}
	if (W_out) *W_out = std::isfinite(W) ? W : 0.0;
	if (n_sel_out) *n_sel_out = nsel;
	if (!std::isfinite(W)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_light_table: the weights' sum is not finite");
	if (!(W > 0.0))
	{
		for (int i = 0; i < n; i++) { if (q) q[i] = 0.f; if (alias) alias[i] = i; if (pmf) pmf[i] = 0.f; }
		return JP_OK;
	}
	std::vector<double> p((size_t)n); std::vector<int> small, large, al((size_t)n); std::vector<float> th((size_t)n);
	small.reserve((size_t)n); large.reserve((size_t)n);
	for (int i = 0; i < n; i++) { p[i] = w[i] * (double)n / W; al[i] = i; th[i] = 1.f; }
	for (int i = n - 1; i >= 0; i--) if (w[i] > 0.0 && p[i] < 1.0) small.push_back(i);
	for (int i = n - 1; i >= 0; i--) if (w[i] == 0.0) small.push_back(i);          // on top of the stack: taken first
	for (int i = n - 1; i >= 0; i--) if (p[i] >= 1.0) large.push_back(i);
	while (!small.empty() && !large.empty())
	{
		const int s = small.back(); small.pop_back();
		const int l = large.back();
		th[s] = (float)p[s]; al[s] = l;
		p[l] = (p[l] + p[s]) - 1.0;
		if (p[l] < 1.0) { large.pop_back(); small.push_back(l); }
	}
	// what is left has its whole bin (threshold 1): bins above average, and bins that rounding left a hair below it.  A bin of weight 0 left
	// here would mean every positive weight was used up first, which the order above excludes; refused rather than made selectable.
	for (int s : small) if (w[s] == 0.0) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_light_table: weights too extreme for the table");
	for (int i = 0; i < n; i++)
	{
		if (q) q[i] = th[i];
		if (alias) alias[i] = al[i];
		if (pmf) pmf[i] = (float)(w[i] / W);
	}
	return JP_OK;
}

// ---- environment map (jp_env.h; INTEGRATION.md "Environment maps"): the check and the tables, in double from the tinted fp32 texels ------
int check_environment_map(const char* who, const JpEnvMap* m)
{
	const std::string w(who);
	if (m->struct_bytes < (int32_t)sizeof(JpEnvMap)) return fail(JP_ERR_INVALID_ARGUMENT, w + ": set JpEnvMap.struct_bytes to sizeof(JpEnvMap)");
	if (m->width < 1 || m->width > 4096 || m->height < 1 || m->height > 4096) return fail(JP_ERR_INVALID_ARGUMENT, w + ": map size out of range (1 .. 4096 per side)");
	if (m->up_axis != JP_ENV_UP_Z && m->up_axis != JP_ENV_UP_Y) return fail(JP_ERR_INVALID_ARGUMENT, w + ": unknown up_axis");
	if (m->importance != 0 && m->importance != -1) return fail(JP_ERR_INVALID_ARGUMENT, w + ": importance must be 0 or -1");
	if (!m->rgb) return fail(JP_ERR_INVALID_ARGUMENT, w + ": null rgb");
	const size_t n = 3 * (size_t)m->width * m->height;
	for (size_t i = 0; i < n; i++) if (!(m->rgb[i] >= 0.f) || !std::isfinite(m->rgb[i])) return fail(JP_ERR_INVALID_ARGUMENT, w + ": a texel value is negative or not finite");
	return JP_OK;
}
struct EnvTables
{
	std::vector<double> weight; std::vector<float> q; std::vector<int32_t> alias; std::vector<float4> texel; std::vector<float2> row_cos;
	double total = 0.0, mean_sum = 0.0; int n_selectable = 0;
};
// texel = tint * map in fp32; Omega_r = (2 pi / W) (ct_r - cb_r); w_t = ((R + G) + B) Omega_r (importance -1: Omega_r); the alias table is build_light_table's
int build_environment_table(const JpEnvMap* m, const float* tint, EnvTables& e)
{
	if (const int st = check_environment_map("jp_build_environment_table", m); st != JP_OK) return st;
	for (int k = 0; k < 3; k++) if (!(tint[k] >= 0.f) || !std::isfinite(tint[k])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_environment_table: the tint is negative or not finite");
	const double kPi = 3.14159265358979323846;
	const int W = m->width, H = m->height; const size_t n = (size_t)W * H;
	e.weight.resize(n); e.q.resize(n); e.alias.resize(n); e.texel.resize(n); e.row_cos.resize((size_t)H);
	std::vector<double> omega((size_t)H);
	double lum = 0.0;
	for (int r = 0; r < H; r++)
	{
		const double ct = std::cos(kPi * (double)r / (double)H), cb = std::cos(kPi * (double)(r + 1) / (double)H);
		omega[r] = (2.0 * kPi / (double)W) * (ct - cb);
		e.row_cos[r] = make_float2((float)ct, (float)cb);
		for (int c = 0; c < W; c++)
		{
			const size_t t = (size_t)r * W + c;
			const float R = tint[0] * m->rgb[3 * t], G = tint[1] * m->rgb[3 * t + 1], B = tint[2] * m->rgb[3 * t + 2];
			if (!std::isfinite(R) || !std::isfinite(G) || !std::isfinite(B)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_build_environment_table: tint x texel is not finite");
			const double s = (((double)R + (double)G) + (double)B) * omega[r];
			lum += s;
			e.weight[t] = m->importance == -1 ? omega[r] : s;
			e.texel[t] = make_float4(R, G, B, 0.f);
		}
	}
	if (const int st = build_light_table((int)n, e.weight.data(), e.q.data(), e.alias.data(), nullptr, &e.total, &e.n_selectable); st != JP_OK) return st;
	if (e.total > 0.0) for (size_t t = 0; t < n; t++) e.texel[t].w = (float)((e.weight[t] / e.total) / omega[t / (size_t)W]);
	e.mean_sum = lum / (4.0 * kPi);
	return JP_OK;
}

// ---- the plan: a pure function of the scene, the options and the sizes the builders (host or device) arrived at ------------------------
// Fills every scalar of the plan; the caller binds the views (sv, tv, pv) to its device tables.
ScenePlan plan_scene(const JpScene* s, const JpOptions& op, bool pick, bool device_build, const PlanSizes& z)
{
	ScenePlan p;
	const bool ref_sem = !device_build && s->bvh_reference_semantics != 0;
	p.cert = z.use_cert;
	p.use_q4 = z.use_q4; p.q4_shadow = z.use_q4 && opt_flag(op.q4_shadow, true);   // shadow rays too (measured against the 8-wide tree: k_shadow 53.8 -> 52.7 ms per 512 spp, frame +4 %)
	p.stack_depth = std::max(2, z.height + 2);                       // binary / 8-wide / verbatim walks: the tree's height
	p.stack_depth_q4 = (z.use_q4 || z.use_cert) ? 3 * z.q4_height + 2 : 0;   // 4-wide walks (Walker<4> / <6>): a node pushes up to three children
	const size_t scene_bytes = ((size_t)z.n_nodes + (size_t)z.n_prims) * 5 * sizeof(float4);   // 80-byte LDS record stride
	const size_t prim_bytes = (size_t)z.n_prims * 5 * sizeof(float4);
	const size_t stack_bytes = (size_t)p.stack_depth * JP_BLOCK * sizeof(int);
	p.scene_in_lds = !device_build && scene_bytes + stack_bytes <= 40 * 1024;   // device-built trees are indexed sparsely (Karras numbering): global memory only
	p.trav_mode = z.use_wide ? 3 : ((z.n_flat > 0 && prim_bytes <= 40 * 1024) ? 2 : (p.scene_in_lds ? 1 : 0));
	if (!z.use_wide && op.traversal > 0) { const int m = op.traversal - 1; if (m == 0 || (m == 1 && p.scene_in_lds)) p.trav_mode = m; }   // experiments: force a lower mode
	if (z.use_wide) p.scene_in_lds = false;
	if (ref_sem) p.trav_mode = 5;
	// large scenes: closest-hit rays walk the binary tree (exact near-to-far order, early out), any-hit shadow rays the
	// 8-wide quantised tree (fewest node fetches; order irrelevant).  Measured on the 280k-triangle scene:
	// k_extend 10.3 ms binary vs 13.8 ms wide, k_shadow 10.6 ms binary vs 8.6 ms wide.
	p.lds_bytes = p.trav_mode == 2 ? prim_bytes : (p.trav_mode == 1 ? stack_bytes + scene_bytes : stack_bytes);
	p.lds_bytes_shadow = p.trav_mode == 3 ? (size_t)2 * (z.wide_height + 2) * JP_BLOCK * sizeof(int) : p.lds_bytes;
	{
		const int planes = pick ? std::min(z.planes, 1) : z.planes;
		size_t tab = ((pick ? (size_t)0 : (size_t)2 * s->n_lights) + (size_t)4 * s->n_materials) * sizeof(float4) + (size_t)s->n_materials * sizeof(int) + 16;
		p.tables_in_lds = tab <= 16 * 1024;
		// k_shade's static LDS (tile index, keys, counters of the material sort) + tables + staging must stay within 64 KB a workgroup;
		// beyond 24 KB of tables the kernel's three workgroups per CU would not fit the CU's LDS either
		const size_t shade_static = (size_t)JP_SHADE_TILE * 3 + (size_t)JP_SHADE_CLASSES * (JP_SHADE_TILE / JP_BLOCK) * (JP_BLOCK / 64) * 4 + 128;
		const size_t prim_part = (size_t)z.n_prims * (4 * sizeof(float4) + sizeof(int4) + 3 * sizeof(float4));     // records, meta, shading frames
		p.shade_prims_in_lds = p.tables_in_lds && p.scene_in_lds && tab + prim_part <= 24 * 1024;
		p.shade_lds_bytes = p.tables_in_lds ? tab + (p.shade_prims_in_lds ? prim_part : 0) : 0;
		const size_t stage_bytes = 16 + (size_t)std::max(1, planes) * 2 * JP_BLOCK * sizeof(float4);
		p.stage_nee = p.tables_in_lds && std::max(1, planes) <= 4 && shade_static + p.shade_lds_bytes + stage_bytes <= 64 * 1024;
		if (p.stage_nee) p.shade_lds_bytes += stage_bytes;
		p.n_planes = std::max(1, planes);
	}
	// material sort in k_shade: pays when the primitives carry more than one material kind (JETPBRT_SHADE_SORT = 0 / 1 forces it)
	bool kinds[8] = { false, false, false, false, false, false, false, false }; int nk = 0;
	for (int i = 0; i < s->n_primitives; i++) { const int m = s->prim_material[i]; const int k = m < 0 ? 7 : s->mat_type[m]; if (!kinds[k]) { kinds[k] = true; nk++; } }
	p.stack_lds_words = op.stack_lds_words >= 2 ? (op.stack_lds_words & ~1) : 12;   // even: the wide tree's entries are word pairs
	// lane refill in the traversal kernels (k_extend_persist / k_shadow_persist): on by default for scenes walked through global
	// memory (measured on the 280k-triangle scene: k_extend 39.1 -> 28.4 ms, k_shadow 28.8 -> 18.9 ms per 128 spp; reference-tree
	// mode 154 -> 227 Msamples/s); the LDS-resident Cornell box loses with it (reference-tree mode 1109 -> 965), so small scenes keep
	// the one-ray-per-lane kernels.  JETPBRT_PERSIST = 0 (off) or the refill threshold (8 / 16 / 32 idle lanes).
	p.persist = ((p.trav_mode == 0 || p.trav_mode == 3 || p.trav_mode == 5) && s->n_primitives > 1024) ? 16 : 0;
	if (op.persist != 0) p.persist = op.persist < 0 ? 0 : op.persist;
	// each iteration the lanes of a wave vote on the kind of step it runs (node / leaf); measured on the 280k-triangle scene: k_extend
	// 28.3 -> 21.9 ms, k_shadow 18.9 -> 16.5 ms per 128 spp.  The reference-tree walk (one node per step, leaf objects as their own
	// steps) is faster without it: 310 vs 286 Msamples/s.
	p.vote = opt_flag(op.vote, p.trav_mode != 5 || p.cert);
	p.class_mask = 1; for (int k = 0; k < 5; k++) if (kinds[k]) p.class_mask |= 2 << k;
	p.shade_sort = opt_flag(op.shade_sort, nk > 1);
	// the rest of the feature set (jp_device.h "Feature sets"; the materials' part is class_mask): shape types of the primitives, light
	// types, shape types under the area lights -- fixed for every frame rendered from this upload, read by the selectors of jp_render.h
	p.shape_mask = 0; p.light_mask = 0; p.light_shape_mask = 0;
	for (int i = 0; i < s->n_primitives; i++) p.shape_mask |= 1 << (s->prim_shape_type[i] & 3);
	for (int i = 0; i < s->n_lights; i++)
	{   // a black light is never sampled (k_shade skips it before sample_li, its two draws kept) and adds nothing on a miss: it is no feature
		const float* rad = s->light_radiance + 3 * i;
		if (rad[0] == 0.f && rad[1] == 0.f && rad[2] == 0.f) continue;
		p.light_mask |= 1 << (s->light_type[i] & 3);
		if (s->light_type[i] == JP_LIGHT_AREA) p.light_shape_mask |= 1 << (s->prim_shape_type[s->light_prim[i]] & 3);
	}
	p.has_null_material = z.has_null;
	return p;
}
}
