// tools/upload_host_check.cpp -- the upload's host half (csrc/jp_scene_host.h: check_scene, build_host_tables, plan_scene) as a stand-alone program for
// AddressSanitizer / UBSan: it needs no context and no device, so nothing is loaded into Python and nothing runs on a GPU.  From the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Wno-unused-value -Xarch_host -fsanitize=address,undefined -Iinclude -Ijet-pbrt_amd/csrc tools/upload_host_check.cpp -o upload_host_check
//   ./upload_host_check        (prints one line per variant, exit status 0)
// The scene: 32 triangles in a row, a root with two 16-triangle leaves, one matte material, triangle 0 an area light; uploaded as acceleration only,
// with the 8-wide tree forced (the leaves are too large for it: the fallback path) and with reference semantics.
#include "jp_common.h"
#include "jp_tex.h"
#include "jp_xbsdf.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include "jp_devmem.h"
#define JP_SHADE_TILE 8192              // as jp_kernels.hip defines it for k_shade
#include "jp_runtime.h"
#include "jp_scene_host.h"

int main()
{
	const int N = 32;
	std::vector<float> p0, p1, p2, nn;
	for (int i = 0; i < N; i++)
	{
		const float x = (float)i;
		const float a[3] = { x, 0, 0 }, b[3] = { x + 0.9f, 0, 0 }, c[3] = { x, 1, 0.1f * i }, n[3] = { 0, 0, 1 };
		p0.insert(p0.end(), a, a + 3); p1.insert(p1.end(), b, b + 3); p2.insert(p2.end(), c, c + 3); nn.insert(nn.end(), n, n + 3);
	}
	std::vector<int> type(N, JP_SHAPE_TRIANGLE), index(N), mat(N, 0), light(N, -1), prim_index(N);
	for (int i = 0; i < N; i++) index[i] = prim_index[i] = i;
	light[0] = 0;
	const int mat_type[1] = { JP_MAT_MATTE }; float mat_params[JP_MAT_PARAM_STRIDE] = { 0.5f, 0.5f, 0.5f };
	const int light_type[1] = { JP_LIGHT_AREA }, light_prim[1] = { 0 }; const float radiance[3] = { 5, 5, 5 };
	const float bounds[18] = { 0, 0, 0, 32, 1, 3.1f, 0, 0, 0, 16, 1, 1.5f, 16, 0, 0, 32, 1, 3.1f };
	const int left[3] = { 1, -1, -17 }, right[3] = { 2, 16, 16 };
	JpScene s; std::memset(&s, 0, sizeof(s));
	s.camera.pos[2] = 10; s.camera.front[2] = -1; s.camera.right[0] = 1; s.camera.up[1] = 1; s.camera.res_x = 32; s.camera.res_y = 24;
	s.n_triangles = N; s.tri_p0 = p0.data(); s.tri_p1 = p1.data(); s.tri_p2 = p2.data(); s.tri_n = nn.data();
	s.n_primitives = N; s.prim_shape_type = type.data(); s.prim_shape_index = index.data(); s.prim_material = mat.data(); s.prim_light = light.data();
	s.n_materials = 1; s.mat_type = mat_type; s.mat_params = mat_params;
	s.n_lights = 1; s.light_type = light_type; s.light_radiance = radiance; s.light_prim = light_prim; s.world_radius = 20;
	s.n_bvh_nodes = 3; s.bvh_bounds = bounds; s.bvh_left = left; s.bvh_right = right; s.n_bvh_prim_indices = N; s.bvh_prim_index = prim_index.data();
	struct Variant { const char* name; int semantics, traversal; bool pick; int mode; } variants[] = { { "plain", 0, 0, false, 2 }, { "wide forced", 0, 4, true, 2 }, { "reference", 1, 0, false, 5 } };
	for (const Variant& v : variants)
	{
		JpOptions op; std::memset(&op, 0, sizeof(op)); op.traversal = v.traversal;
		s.bvh_reference_semantics = v.semantics;
		SceneCheck k; HostTables t;
		if (check_scene(&s, v.pick, k) != JP_OK || build_host_tables(&s, op, v.pick, k, t) != JP_OK) { std::printf("%s: %s\n", v.name, g_err.c_str()); return 1; }
		const ScenePlan p = plan_scene(&s, op, v.pick, false, t.sizes());
		TableBytes tb[TAB_COUNT]; t.tables(tb);
		unsigned long long h = 0; for (const TableBytes& b : tb) if (b.present) h ^= fnv1a(b.data, b.bytes);
		std::printf("%-12s mode %d, %d nodes, %zu records, %zu flat boxes, height %d, tables %016llx\n", v.name, p.trav_mode, t.n_nodes, t.meta.size(), t.flat.size() / 2, k.height, h);
		if (p.trav_mode != v.mode || (int)t.meta.size() != N || k.n_leaves != 2 || t.use_wide) return 1;
	}
	s.bvh_prim_index = nullptr;                                        // and one refusal
	SceneCheck k;
	return check_scene(&s, false, k) == JP_ERR_INVALID_ARGUMENT ? 0 : 1;
}
