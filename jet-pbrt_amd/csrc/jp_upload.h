// jet-pbrt_amd/csrc/jp_upload.h -- host runtime, part 2 of 3: jp_upload_scene -- check (jp_scene_host.h: every index validated on the host) -> tables (the host
// builders of jp_scene_host.h, or the device-side hierarchy build of jp_lbvh.h / jp_ploc.h) -> uploads -> plan (plan_scene) -> views.  The tables go into a LOCAL
// SceneTables through upload() or are moved there out of the builders' results, and reach the context only once everything has succeeded; nothing here frees by hand.
// jp_describe_upload runs the host half of the same sequence without a device.  Included by jp_kernels.hip after jp_scene_host.h.
#pragma once
namespace
{
// ---- no hierarchy handed over: records go up in creation order and the trees are built on the device (jp_lbvh.h, jp_ploc.h) ----------
int device_build_tables(JpContext* c, const JpScene* s, bool pick, const SceneCheck& k, HostTables& t, SceneTables& T, float& build_ms)
{
	const JpOptions& op = c->opt;
	if (const int st = check_leaf_encoding(s); st != JP_OK) return st;
	RecordEmitter em(s, op, t);
	t.device_build = true; t.has_null = k.has_null;
	for (int p = 0; p < s->n_primitives; p++) em.emit_prim(p);
	DevBuf p0, m0; float4* d_p0; int4* d_m0;                    // the records in creation order: only the builders read them
	hipError_t e = reserve(p0, d_p0, t.prims.size() * sizeof(float4)); if (e == hipSuccess) e = reserve(m0, d_m0, t.meta.size() * sizeof(int4));
	if (e == hipSuccess) e = hipMemcpyAsync(d_p0, t.prims.data(), t.prims.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_m0, t.meta.data(), t.meta.size() * sizeof(int4), hipMemcpyHostToDevice, c->stream);
	LbvhResult lr; std::vector<int> sorted;
	// leaf size: LBVH 3 (round 1, 280k-triangle scene: 540 / 578 / 579 / 560 / 534 / 497 Msamples/s for 1 / 2 / 3 / 4 / 6 / 8); PLOC 2 (round 3, with the 4-wide
	// tree: k_extend 28.0 / 25.3 / 26.1 / 27.1 ms and k_shadow 21.7 / 19.8 / 20.5 / 21.6 ms per 256 spp for 1 / 2 / 3 / 4, profiles/r03g_ploc_ab.txt)
	bool ploc = op.device_tree != 2;
	int maxLeaf = ploc ? 2 : 3;
	if (op.bvh_max_leaf >= 1 && op.bvh_max_leaf <= 16) maxLeaf = op.bvh_max_leaf;
	// [round 3] PLOC clustering (jp_ploc.h) instead of the Karras topology; JETPBRT_DEVICE_TREE=lbvh restores the latter, which also serves
	// as the fallback should the clustering not finish within its round limit
	if (e == hipSuccess && ploc) { e = ploc_build(c->stream, d_p0, d_m0, s->n_primitives, maxLeaf, op.ploc_radius, op.ploc_max_rounds, lr, sorted); if (e == hipErrorNotReady) { e = hipSuccess; ploc = false; } }
	if (e == hipSuccess && !ploc) e = lbvh_build(c->stream, d_p0, d_m0, s->n_primitives, maxLeaf, lr, sorted);
	p0.reset(); m0.reset();
	if (e != hipSuccess) return fail(JP_ERR_DEVICE, std::string("jp_upload_scene: device BVH build failed: ") + hipGetErrorString(e));
	if (lr.height + 2 > 60) return fail(JP_ERR_UNSUPPORTED, "jp_upload_scene: device-built BVH is deeper than the 58-entry traversal stack; hand over a host-built hierarchy for this scene");
	T.nodes = std::move(lr.nodes); T.prims = std::move(lr.prims); T.meta = std::move(lr.meta);
	for (int i = 0; i < s->n_primitives; i++) t.devPrimOf[sorted[i]] = i;
	t.height = lr.height; build_ms = lr.build_ms; t.n_nodes = lr.n_nodes;
	// the 8-wide tree for the shadow rays, collapsed from the binary tree on the device as well (jp_lbvh.h)
	const bool want_wide = opt_flag(op.device_wide, s->n_primitives > 64);
	if (want_wide)
	{
		WideResult wr;
		e = lbvh_build_wide(c->stream, T.nodes.get<float4>(), s->n_primitives, wr);
		if (e != hipSuccess) return fail(JP_ERR_DEVICE, std::string("jp_upload_scene: device wide-tree build failed: ") + hipGetErrorString(e));
		if (wr.wide) { T.wide = std::move(wr.wide); t.n_wide = wr.n_wide; t.wide_height = wr.height; t.use_wide = true; build_ms += wr.build_ms; }
	}
	// [round 3] ... and the 4-wide tree of Walker<4> for the closest-hit (and shadow) rays, as the host path has it
	const bool want_q4 = s->n_primitives > 1024 && opt_flag(op.q4, true);
	if (want_q4)
	{
		WideResult qr;
		e = lbvh_build_q4(c->stream, T.nodes.get<float4>(), s->n_primitives, qr);
		if (e != hipSuccess) return fail(JP_ERR_DEVICE, std::string("jp_upload_scene: device 4-wide tree build failed: ") + hipGetErrorString(e));
		if (qr.wide) { T.q4 = std::move(qr.wide); t.n_q4 = qr.n_wide; build_ms += qr.build_ms; t.use_q4 = true; t.q4_height = qr.height; }
	}
	build_material_light_tables(s, pick, t);
	build_shade_tab(s, pick, t);
	return JP_OK;
}

// the view every kernel takes: pointers into the device tables, counts and scalars from the builders
void bind_scene_view(SceneView& v, const SceneTables& T, const HostTables& t, const JpScene* s)
{
	v.nodes = T.nodes.get<float4>(); v.n_nodes = t.n_nodes;
	v.prims = T.prims.get<float4>(); v.meta = T.meta.get<int4>(); v.n_prims = (int)t.meta.size();
	v.mats = T.mats.get<float4>(); v.mat_type = T.mat_type.get<int>(); v.n_mats = s->n_materials;
	v.lights = T.lights.get<float4>(); v.n_lights = s->n_lights; v.shade_tab = T.shade_tab.get<float4>();
	v.env_sum = make_float3(t.env_sum[0], t.env_sum[1], t.env_sum[2]); v.n_env = t.n_env;
	v.world_radius = s->world_radius; v.cam = s->camera;
	v.flat = T.flat.get<float4>(); v.n_flat = (int)(t.flat.size() / 2);
	v.wide = T.wide.get<uint4>(); v.n_wide = t.n_wide;
	v.q4 = T.q4.get<uint4>(); v.n_q4 = t.n_q4;
	v.refbox = T.refbox.get<float4>(); v.cert_pad = t.cert_pad; v.cert_pad_eye = t.cert_pad_eye;
}
}

extern "C" int jp_upload_scene(JpContext* c, const JpScene* s)
{
	if (!c || !s) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene: null argument");
	const bool pick = c->light_mode == JP_LIGHTS_POWER_ONE;
	SceneCheck k;
	if (const int st = check_scene(s, pick, k); st != JP_OK) return st;
	const int n_textures = c->upload_n_textures; c->upload_n_textures = 0;   // (jp_upload_scene_textured's count; a plain upload has none)
	if (const int st = check_sampling_counts(c, n_textures); st != JP_OK) return st;   // jp_set_texture_sampling: refused while the old scene is still there
	if (const int st = check_mipmap_counts(c, n_textures); st != JP_OK) return st;     // jp_set_texture_mipmaps: likewise
	if (const int st = check_procedural_counts(c, n_textures); st != JP_OK) return st; // jp_set_texture_procedurals: likewise
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	free_scene(c);                                                  // first: the old and the new scene are never resident together

	// from here on a failure leaves the context without a scene: the new tables are local until the last step
	HostTables t; SceneTables T; float build_ms = 0.f;
	if (const int st = k.device_build ? device_build_tables(c, s, pick, k, t, T, build_ms) : build_host_tables(s, c->opt, pick, k, t); st != JP_OK) return st;
	static DevBuf SceneTables::* const kDst[TAB_COUNT] = { &SceneTables::nodes, &SceneTables::prims, &SceneTables::meta, &SceneTables::mats, &SceneTables::mat_type, &SceneTables::lights,
	                                                        &SceneTables::shade_tab, &SceneTables::wide, &SceneTables::q4, &SceneTables::refbox, &SceneTables::flat };
	TableBytes tb[TAB_COUNT]; t.tables(tb);
	for (int i = 0; i < TAB_COUNT; i++) if (tb[i].present) HIP_TRY(upload(T.*kDst[i], tb[i].data, tb[i].bytes));
	ScenePlan p = plan_scene(s, c->opt, pick, k.device_build, t.sizes());
	bind_scene_view(p.sv, T, t, s);
	if (c->env_map.W > 0) { if (const int st = upload_environment_map(c, T, p, s, pick); st != JP_OK) return st; c->env_importance = c->env_map.importance; }   // before the light table, which weighs the map light
	if (pick) if (const int st = upload_light_table(c, T, p, s, t.light_area); st != JP_OK) return st;
	if (c->vnormals.set) if (const int st = upload_vertex_normals(c, T, p, s); st != JP_OK) return st;   // (a scene whose normals are all flat keeps its plan)
	if (c->nmaps.set) if (const int st = upload_normal_maps(c, T, p, s); st != JP_OK) return st;          // (so does a scene whose maps perturb nothing)
	if (const int st = upload_map_sampling(c, T, p); st != JP_OK) return st;                              // (... and a scene whose maps' sampling records are all the identity)

	c->tab = std::move(T); c->plan = p; c->plan.have_scene = true;
	c->build_on_device = k.device_build; c->build_ms = build_ms; c->bvh_height = t.height; c->bvh_nodes = k.ref_sem ? s->n_bvh_nodes : t.n_nodes;
	c->cert_eye_leaves = t.eye_leaves; c->cert_fell_back = false;
	// what jp_read_scene_table / jp_get_tree_info hand back: the bytes of every table in use (a device build's buffers are sized for the worst case) and the wide heights
	for (int i = 0; i < TAB_COUNT; i++) c->tab_bytes[i] = tb[i].present ? tb[i].bytes : 0;
	if (k.device_build)
	{
		c->tab_bytes[TAB_NODES] = (size_t)t.n_nodes * 4 * sizeof(float4); c->tab_bytes[TAB_PRIMS] = (size_t)s->n_primitives * 4 * sizeof(float4); c->tab_bytes[TAB_META] = (size_t)s->n_primitives * sizeof(int4);
		c->tab_bytes[TAB_WIDE] = (size_t)t.n_wide * 20 * sizeof(uint32_t); c->tab_bytes[TAB_Q4] = (size_t)t.n_q4 * 16 * sizeof(uint32_t);
	}
	c->wide_height = t.wide_height; c->q4_height = t.q4_height;
	return JP_OK;
}

// What jp_upload_scene would decide for this scene, and the bytes it would hand to the device -- check_scene, build_host_tables and plan_scene, no device
namespace
{
// the host half of an upload for the two entry points that run it without a device: options, check, tables (the plan is the caller's)
int host_upload_tables(const std::string& who, const JpOptions* o, int32_t light_mode, const JpScene* s, JpOptions& op, SceneCheck& k, HostTables& t)
{
	if (light_mode != JP_LIGHTS_ALL && light_mode != JP_LIGHTS_POWER_ONE) return fail(JP_ERR_INVALID_ARGUMENT, who + ": unknown light sampling mode");
	std::memset(&op, 0, sizeof(op)); op.struct_bytes = (int32_t)sizeof(JpOptions);                   // NULL: the defaults, no environment
	if (o) if (const int st = read_options(who.c_str(), o, op); st != JP_OK) return st;
	const bool pick = light_mode == JP_LIGHTS_POWER_ONE;
	if (const int st = check_scene(s, pick, k); st != JP_OK) return st;
	if (k.device_build) return fail(JP_ERR_UNSUPPORTED, who + ": a scene without a hierarchy (n_bvh_nodes == 0) gets its trees from the device builders");
	return build_host_tables(s, op, pick, k, t);
}
}

extern "C" int jp_describe_upload(const JpOptions* o, int32_t light_mode, const JpScene* s, JpUploadInfo* out)
{
	if (!s || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_describe_upload: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_describe_upload: set JpUploadInfo.struct_bytes to sizeof(JpUploadInfo)");
	JpOptions op; SceneCheck k; HostTables t;
	if (const int st = host_upload_tables("jp_describe_upload", o, light_mode, s, op, k, t); st != JP_OK) return st;
	const bool pick = light_mode == JP_LIGHTS_POWER_ONE;
	const ScenePlan p = plan_scene(s, op, pick, false, t.sizes());
	JpUploadInfo i; std::memset(&i, 0, sizeof(i));
	i.trav_mode = p.trav_mode; i.stack_depth = p.stack_depth; i.stack_depth_q4 = p.stack_depth_q4;
	i.lds_bytes = (int64_t)p.lds_bytes; i.lds_bytes_shadow = (int64_t)p.lds_bytes_shadow; i.shade_lds_bytes = (int64_t)p.shade_lds_bytes;
	i.scene_in_lds = p.scene_in_lds; i.tables_in_lds = p.tables_in_lds; i.shade_prims_in_lds = p.shade_prims_in_lds; i.stage_nee = p.stage_nee; i.n_planes = p.n_planes;
	i.persist = p.persist; i.vote = p.vote; i.shade_sort = p.shade_sort; i.use_q4 = p.use_q4; i.q4_shadow = p.q4_shadow; i.cert = p.cert;
	i.class_mask = p.class_mask; i.shape_mask = p.shape_mask; i.light_mask = p.light_mask; i.light_shape_mask = p.light_shape_mask;
	i.has_null_material = p.has_null_material; i.stack_lds_words = p.stack_lds_words;
	i.n_nodes = t.n_nodes; i.n_prims = (int32_t)t.meta.size(); i.n_flat = (int32_t)(t.flat.size() / 2); i.n_wide = t.n_wide; i.n_q4 = t.n_q4;
	i.bvh_nodes = k.ref_sem ? s->n_bvh_nodes : t.n_nodes; i.bvh_height = t.height; i.wide_height = t.wide_height; i.q4_height = t.q4_height;
	i.cert_eye_leaves = p.cert ? t.eye_leaves : 0; i.n_env = t.n_env;
	i.cert_pad = t.cert_pad; i.cert_pad_eye = t.cert_pad_eye; std::memcpy(i.env_sum, t.env_sum, sizeof(i.env_sum));
	TableBytes tb[TAB_COUNT]; t.tables(tb);
	for (int j = 0; j < TAB_COUNT; j++) if (tb[j].present) { i.table[j].bytes = (int64_t)tb[j].bytes; i.table[j].fnv1a = fnv1a(tb[j].data, tb[j].bytes); }
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);                                                   // (a shorter struct of the caller is truncated)
	return JP_OK;
}

// The bytes behind one entry of JpUploadInfo.table: the same options, check and builders, then the table the upload would copy to the device
extern "C" int jp_copy_upload_table(const JpOptions* o, int32_t light_mode, const JpScene* s, int32_t which, void* out, int64_t capacity_bytes, int64_t* bytes)
{
	if (!s || !bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_copy_upload_table: null argument");
	if (which < 0 || which >= TAB_COUNT) return fail(JP_ERR_INVALID_ARGUMENT, "jp_copy_upload_table: no such table");
	JpOptions op; SceneCheck k; HostTables t;
	if (const int st = host_upload_tables("jp_copy_upload_table", o, light_mode, s, op, k, t); st != JP_OK) return st;
	TableBytes tb[TAB_COUNT]; t.tables(tb);
	*bytes = tb[which].present ? (int64_t)tb[which].bytes : 0;
	if (!out) return JP_OK;                                                    // the size only
	if (capacity_bytes < *bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_copy_upload_table: capacity_bytes smaller than the table");
	if (*bytes > 0) std::memcpy(out, tb[which].data, (size_t)*bytes);
	return JP_OK;
}

// ---- the uploaded scene's hierarchy tables back on the host (tests: tests/tree_ref.py validates them), and the counts and heights that go with them
extern "C" int jp_read_scene_table(JpContext* c, int32_t which, void* out, int64_t capacity_bytes, int64_t* bytes)
{
	if (!c || !bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_scene_table: null argument");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_read_scene_table: no scene uploaded");
	const DevBuf* src = which == TAB_NODES ? &c->tab.nodes : which == TAB_PRIMS ? &c->tab.prims : which == TAB_META ? &c->tab.meta : which == TAB_WIDE ? &c->tab.wide
	                  : which == TAB_Q4 ? &c->tab.q4 : which == TAB_FLAT ? &c->tab.flat : nullptr;
	if (!src) return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_scene_table: not a hierarchy table (nodes, prims, meta, wide, q4, flat)");
	*bytes = (int64_t)c->tab_bytes[which];
	if ((size_t)*bytes > src->bytes()) return fail(JP_ERR_DEVICE, "jp_read_scene_table: the table is larger than its device buffer");
	if (!out) return JP_OK;                                                    // the size only
	if (capacity_bytes < *bytes) return fail(JP_ERR_INVALID_ARGUMENT, "jp_read_scene_table: capacity_bytes smaller than the table");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (*bytes > 0) HIP_TRY(hipMemcpy(out, src->get<void>(), (size_t)*bytes, hipMemcpyDeviceToHost));
	return JP_OK;
}
extern "C" int jp_get_tree_info(JpContext* c, JpTreeInfo* out)
{
	if (!c || !out) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_tree_info: null argument");
	if (out->struct_bytes < (int32_t)sizeof(int32_t)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_get_tree_info: set JpTreeInfo.struct_bytes to sizeof(JpTreeInfo)");
	if (!c->plan.have_scene) return fail(JP_ERR_NO_SCENE, "jp_get_tree_info: no scene uploaded");
	const SceneView& v = c->plan.sv;
	JpTreeInfo i; std::memset(&i, 0, sizeof(i));
	i.n_prims = v.n_prims; i.n_nodes = v.n_nodes; i.bvh_height = c->bvh_height;
	i.n_wide = v.n_wide; i.wide_height = c->wide_height; i.n_q4 = v.n_q4; i.q4_height = c->q4_height; i.n_flat = v.n_flat;
	const size_t n = std::min((size_t)out->struct_bytes, sizeof(i));
	i.struct_bytes = (int32_t)n;
	std::memcpy(out, &i, n);
	return JP_OK;
}


// ---- textures: validation on the host, then the scene, then the texture tables (TexView) ------------------------------------------
namespace
{
// every index and size of `t` against the scene.  pool: texels of the device pool (RGBA8); ntm: materials that use a texture
int check_textures(const JpScene* s, const JpTextures* t, long long& pool, int& ntm)
{
	pool = 0; ntm = 0;
	if (t->struct_bytes < (int32_t)sizeof(JpTextures)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: JpTextures.struct_bytes smaller than this library's JpTextures");
	if (t->n_textures < 0 || t->n_textures > (1 << 28)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: n_textures out of range");
	const int nt = t->n_textures;
	if (nt == 0) return JP_OK;                                         // exactly jp_upload_scene: nothing else of `t` is looked at
	if (!t->tex_type || !t->tex_color) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: null tex_type / tex_color");
	if (t->n_materials != s->n_materials) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: n_materials differs from the scene's");
	if (t->n_triangles != s->n_triangles) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: n_triangles differs from the scene's");
	if (t->n_materials > 0 && (!t->mat_texture || !s->mat_type)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: null mat_texture");
	for (int i = 0; i < nt; i++)
	{
		const int ty = t->tex_type[i];
		if (ty < JP_TEXTURE_SOLID || ty > JP_TEXTURE_IMAGE) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: unknown texture type");
		if (ty == JP_TEXTURE_IMAGE)
		{
			if (!t->tex_width || !t->tex_height || !t->tex_offset || !t->texels) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: image texture without tex_width / tex_height / tex_offset / texels");
			const long long w = t->tex_width[i], h = t->tex_height[i], off = t->tex_offset[i];
			if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: image size out of range (1 .. 16384 per side)");
			if (off < 0 || t->n_texel_bytes < 0 || off > t->n_texel_bytes - 3 * w * h) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: image texels beyond n_texel_bytes");
			pool += w * h;
		}
		else
		{
			const int nc = ty == JP_TEXTURE_CHECKER ? 6 : 3;
			for (int k = 0; k < nc; k++) if (!std::isfinite(t->tex_color[6 * (size_t)i + k])) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: colour not finite");
		}
	}
	if (pool > 0x7fffffffll) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: more than 2^31 texels in all");
	for (int m = 0; m < t->n_materials; m++)
	{
		const int k = t->mat_texture[m];
		if (k < -1 || k >= nt) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: mat_texture out of range");
		if (k < 0) continue;
		const int mt = s->mat_type[m];
		if (mt != JP_MAT_MATTE && mt != JP_MAT_MIRROR && mt != JP_MAT_PLASTIC) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: a texture on a glass or metal material (its [0..2] is eta, not a colour)");
		ntm++;
	}
	if (s->n_primitives > 0 && (!s->prim_shape_type || !s->prim_shape_index)) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: null array");
	return JP_OK;
}
struct TexTables { std::vector<int4> desc; std::vector<float4> col; std::vector<unsigned int> texels; std::vector<int> mat_tex; std::vector<float2> prim_uv; };
void build_texture_tables(const JpScene* s, const JpTextures* t, long long pool, TexTables& x)
{
	const int nt = t->n_textures;
	std::vector<int4>& desc = x.desc; std::vector<float4>& col = x.col; std::vector<unsigned int>& texels = x.texels;
	desc.resize(nt); col.resize(2 * (size_t)nt); texels.resize((size_t)pool);
	size_t at = 0;
	for (int i = 0; i < nt; i++)
	{
		const float* cc = t->tex_color + 6 * (size_t)i;
		desc[i] = make_int4(t->tex_type[i], 0, 0, 0);
		col[2 * i] = make_float4(0, 0, 0, 0); col[2 * i + 1] = make_float4(0, 0, 0, 0);
		if (t->tex_type[i] == JP_TEXTURE_IMAGE)
		{
			const int w = t->tex_width[i], h = t->tex_height[i];
			desc[i].y = w; desc[i].z = h; desc[i].w = (int)at;
			const uint8_t* src = t->texels + t->tex_offset[i];
			for (size_t k = 0; k < (size_t)w * h; k++) texels[at + k] = (unsigned int)src[3 * k] | ((unsigned int)src[3 * k + 1] << 8) | ((unsigned int)src[3 * k + 2] << 16) | 0xff000000u;
			at += (size_t)w * h;
		}
		else
		{
			col[2 * i] = make_float4(cc[0], cc[1], cc[2], 0);
			if (t->tex_type[i] == JP_TEXTURE_CHECKER) col[2 * i + 1] = make_float4(cc[3], cc[4], cc[5], 0);
		}
	}
	x.mat_tex.assign(t->mat_texture, t->mat_texture + t->n_materials);
	std::vector<float2>& puv = x.prim_uv; puv.assign(3 * (size_t)s->n_primitives, make_float2(0, 0));
	if (t->tri_uv)
		for (int p = 0; p < s->n_primitives; p++)
			if (s->prim_shape_type[p] == JP_SHAPE_TRIANGLE)
			{
				const float* u = t->tri_uv + 6 * (size_t)s->prim_shape_index[p];
				for (int k = 0; k < 3; k++) puv[3 * (size_t)p + k] = make_float2(u[2 * k], u[2 * k + 1]);
			}
}
}

extern "C" int jp_upload_scene_textured(JpContext* c, const JpScene* s, const JpTextures* t)
{
	if (!c || !s) return fail(JP_ERR_INVALID_ARGUMENT, "jp_upload_scene_textured: null argument");
	if (!t) return jp_upload_scene(c, s);
	long long pool; int ntm;
	if (const int st = check_textures(s, t, pool, ntm); st != JP_OK) return st;
	if (const int st = check_sampling_textures(c, t); st != JP_OK) return st;
	if (const int st = check_mipmap_textures(c, t, pool); st != JP_OK) return st;
	if (const int st = check_procedural_textures(c, t); st != JP_OK) return st;
	c->upload_n_textures = t->n_textures;
	const int st = jp_upload_scene(c, s); c->upload_n_textures = 0;                              // (validates the scene; drops the textures of an earlier upload)
	if (st != JP_OK) return st;
	if (ntm == 0) return JP_OK;                                        // no textures, or textures no material uses: the untextured scene, exactly
	TexTables x; build_texture_tables(s, t, pool, x);
	SceneTables& T = c->tab;
	const long long pool_mip = mip_pool_texels(c, t, pool);             // jp_set_texture_mipmaps: the pool's allocation grows by the pyramids (equal to pool without them)
	if (pool_mip > pool && T.texels.reserve((size_t)pool_mip * sizeof(unsigned int)) != hipSuccess) { free_scene(c); return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: out of device memory for the pyramids"); }
	if (upload(T.tex_desc, x.desc.data(), x.desc.size() * sizeof(int4)) != hipSuccess || upload(T.tex_col, x.col.data(), x.col.size() * sizeof(float4)) != hipSuccess
	    || upload(T.texels, x.texels.data(), x.texels.size() * sizeof(unsigned int)) != hipSuccess || upload(T.mat_tex, x.mat_tex.data(), x.mat_tex.size() * sizeof(int)) != hipSuccess
	    || upload(T.prim_uv, x.prim_uv.data(), x.prim_uv.size() * sizeof(float2)) != hipSuccess)
	{
		free_scene(c);
		return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: out of device memory for the texture tables");
	}
	TexView& tv = c->plan.tv; tv = TexView();
	tv.desc = T.tex_desc.get<int4>(); tv.col = T.tex_col.get<float4>(); tv.texels = T.texels.get<unsigned int>();
	tv.mat_tex = T.mat_tex.get<int>(); tv.prim_uv = T.prim_uv.get<float2>();
	c->plan.textured = true; c->n_textures = t->n_textures; c->n_tex_mats = ntm; c->texel_bytes = (long long)x.texels.size() * 4;
	if (upload_tex_sampling(c, T, c->plan) != JP_OK) { free_scene(c); return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: out of device memory for the sampling records"); }
	if (pool_mip > pool && upload_mipmaps(c, T, c->plan, s, t, x.desc, pool) != JP_OK) { free_scene(c); return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: building the pyramids failed"); }
	if (upload_procedurals(c, T, c->plan, s, t) != JP_OK) { free_scene(c); return fail(JP_ERR_DEVICE, "jp_upload_scene_textured: out of device memory for the procedural records"); }
	return JP_OK;
}
