// oracle/pt_features.cc -- TEST INFRASTRUCTURE ONLY (see pt_oracle.cc).  The second translation unit of libjp_oracle.so: the path integrator of pt_oracle.cc with the
// features the library added on top of the reference -- light selection, environment maps, the MIS estimator, vertex normals, textures, texture sampling records,
// normal maps, the lens, the film state, the ray cone with mip-mapped and procedural textures -- restated from their written definitions (INTEGRATION.md sections 7,
// 9 - 16, 18 and 19), one path at a time.  The reference has
// none of these features; nothing here follows reference code that pt_oracle.cc does not already restate.
//
// What is shared and what is restated:
//   - the restated reference functions of pt_oracle.cc (shapes, tree, BSDFs, sample_li, occluded, the sampler) are used as they are: this file includes that one
//     with its entry points compiled out, so there is one text of them and no symbol is defined twice;
//   - the definition headers under include/ that the device kernels compile too (jp_normals.h, jp_normal_map.h, jp_tex_sampling.h, jp_lens.h, jp_film.h, and of
//     jp_mipmap.h and jp_procedural.h the lookups: jp_mip_lookup_above with its level and fraction, jp_proc_lookup) are included: each has a Python restatement
//     and host tests of its own;
//   - the pyramids arrive as data from jp_build_mip_chain, like the tables;
//   - the tables (light table, map tables) arrive as data from jp_build_light_table / jp_build_environment_table, which have tests of their own;
//   - everything else -- which draw feeds which decision, the pick, the map lookup and its five-draw sample, the strategy pdfs, the power heuristic and where it
//     applies, the carried record behind null-material primitives, which normal enters which product, the geometric-side guard, the uv of each shape, the
//     texture lookups; the path's cone (gamma0, the reset at bounce 0, the step at every hit, which flag and which bounce number a segment carries), the footprint
//     area of each shape and rho with their guards, which lookup a footprint selects, the identity record above level 0, a record's resolved form (defaults, norm,
//     s, antialias off), its precedence on a checker texture and the colour its side word stands for -- is written here from the document.
// Same build as pt_oracle.cc: baseline x86-64, -O2, no contraction.
#define JP_ORACLE_NO_ENTRY_POINTS
#include "pt_oracle.cc"
#include "pt_features.h"
#include "jp_normals.h"
#include "jp_normal_map.h"
#include "jp_tex_sampling.h"
#include "jp_lens.h"
#include "jp_film.h"
#include "jp_mipmap.h"
#include "jp_procedural.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Undecided lookups.  acosf / atan2f / asinf are the only operations of a path the device does not share with this host code bit for bit: it takes them from
// its own math library.  Their results feed a float -> int conversion (the texel of a map lookup, of an image lookup on a sphere or a disk), so a value within
// the two libraries' disagreement of an integer may select the neighbouring texel on the device.
// Margin, in texel units, for a coordinate on an axis of `size` texels: size * 2^-19, that is 32 ulp of the largest coordinate the axis has (a coordinate in
// [size/2, size) has ulp size * 2^-24).  Budget: each library is taken to be within 4 ulp of the true acosf / atan2f / asinf (glibc documents <= 1 ulp for the
// three, the ROCm device library <= 2 ulp; 4 is twice the larger figure), which is 8 ulp of disagreement in the angle; the angle then goes through at most four
// more fp32 operations on each side (+ 2 pi, + pi or + pi / 2, a division by pi or 2 pi, the product with the size or the scale), half an ulp each, 4 ulp in all;
// the angle's own ulp, carried to the coordinate, is at most twice the coordinate's (phi in [pi, 2 pi) over 2 pi times W lies in [W/2, W): same binade; the other
// ranges are more favourable), so 2 * 8 + 4 = 20 ulp <= 32.  Nothing here was tuned on device output.
// Only interior borders count: the coordinate 0 and the coordinate `size` border nothing, both sides clamp to the first and the last texel there, and the sign
// test `phi < 0` is exact on both sides (atan2f returns the sign of y).
// ---------------------------------------------------------------------------------------------
inline float lookup_margin(int size) { return (float)(size > 1 ? size : 1) * 1.9073486328125e-6f; }   // 2^-19
inline bool near_border(float c, int size)
{
	if (!(c - c == 0.f)) return false;                                   // not finite: texel 0 on both sides
	const float k = std::floor(c + 0.5f);
	if (k < 1.f || k > (float)(size - 1)) return false;
	return std::fabs(c - k) <= lookup_margin(size);
}

struct Image { int w, h; std::vector<unsigned int> px; };                // one dword per texel, R | G << 8 | B << 16 (what include/jp_tex_sampling.h addresses)
inline Image load_rgb8(const uint8_t* base, int64_t off, int w, int h)
{
	Image im; im.w = w; im.h = h; im.px.resize((size_t)w * h);
	for (size_t k = 0; k < im.px.size(); k++) { const uint8_t* t = base + off + 3 * k; im.px[k] = (unsigned int)t[0] | ((unsigned int)t[1] << 8) | ((unsigned int)t[2] << 16); }
	return im;
}

// a pyramid as include/jp_mipmap.h's lookup addresses it: every level in one dword pool, level 0 first
struct Pyramid { std::vector<unsigned int> px; std::vector<JpMipLevel> lev; };

// section 19, the record as the lookup reads it: octaves 0 -> 6 (NOISE: 1), gain 0 -> 0.5, variation 0 -> 1; norm = 1 / sum of gain^i over the record's octaves, fp32
// in octave order; s = the square root of the largest squared column norm of M's linear part, 0 with antialias off
inline JpProcDev resolve_record(const JpProcedural& r)
{
	JpProcDev d;
	d.kind = r.kind; d.space = r.space; d.pad = 0;
	d.octaves = r.kind == JP_PROC_NOISE ? 1 : (r.octaves == 0 ? 6 : r.octaves);
	for (int k = 0; k < 12; k++) d.m[k] = r.m[k];
	d.gain = r.gain == 0.f ? 0.5f : r.gain;
	d.variation = r.variation == 0.f ? 1.f : r.variation;
	float sum = 0.f, amp = 1.f;
	for (int i = 0; i < d.octaves; i++) { sum = sum + amp; amp = amp * d.gain; }
	d.norm = 1.f / sum;
	float best = 0.f;
	for (int c = 0; c < 3; c++) { const float n2 = (r.m[c] * r.m[c] + r.m[4 + c] * r.m[4 + c]) + r.m[8 + c] * r.m[8 + c]; if (n2 > best) best = n2; }
	d.s = r.antialias < 0 ? 0.f : std::sqrt(best);
	return d;
}

struct FState
{
	JpOracleFeatures f;
	bool pick, has_map, mis;
	float row_scale, col_scale, phi_step;
	std::vector<Image> tex_img, nmap_img;
	std::vector<char> tri_smooth;
	bool lens_on; JpLensPlan lens;
	bool film_on;
	// sections 18, 19
	std::vector<Pyramid> pyr;                 // per texture; no levels: no pyramid
	std::vector<JpProcDev> proc;              // per texture; kind JP_PROC_NONE: no record
	bool cone;                                // the paths carry a cone: a pyramid or an antialiased record exists
	float gamma0, bounce_spread, footprint_scale;
	const JpTexSampler* tex_rec(int t) const
	{
		if (!f.sampling || !f.sampling->tex || t >= f.sampling->n_textures) return nullptr;
		const JpTexSampler* s = f.sampling->tex + t;
		return jp_tsamp_identity(s, JP_TSAMP_COLOR) ? nullptr : s;
	}
	const JpTexSampler* map_rec(int k) const
	{
		if (!f.sampling || !f.sampling->map || k >= f.sampling->n_maps) return nullptr;
		const JpTexSampler* s = f.sampling->map + k;
		return jp_tsamp_identity(s, JP_TSAMP_NORMAL) ? nullptr : s;
	}
};

int prepare(const JpScene* js, const JpOracleFeatures* in, FState& fs)
{
	std::memset(&fs.f, 0, sizeof(fs.f));
	if (in) std::memcpy(&fs.f, in, std::min((size_t)in->struct_bytes, sizeof(fs.f)));
	const JpOracleFeatures& f = fs.f;
	fs.pick = f.light_mode == JP_LIGHTS_POWER_ONE;
	fs.has_map = f.env_w > 0;
	fs.mis = f.estimator == JP_ESTIMATOR_MIS;
	if (fs.pick && (f.n_lights != js->n_lights || (f.n_lights > 0 && (!f.q || !f.alias || !f.pmf)))) return JP_ERR_INVALID_ARGUMENT;
	if (fs.pick && f.n_env > 0 && !f.env_lights) return JP_ERR_INVALID_ARGUMENT;
	if ((fs.has_map || fs.mis) && !fs.pick) return JP_ERR_UNSUPPORTED;     // sections 10, 11: both need the light table
	if (fs.has_map && (!f.env_texel || !f.env_q || !f.env_alias || !f.env_row_cos || f.env_h < 1 || f.env_light < 0 || f.env_light >= js->n_lights)) return JP_ERR_INVALID_ARGUMENT;
	fs.row_scale = fs.col_scale = fs.phi_step = 0.f;
	if (fs.has_map) { fs.row_scale = (float)f.env_h / kPi; fs.col_scale = (float)f.env_w / k2Pi; fs.phi_step = k2Pi / (float)f.env_w; }
	if (f.textures && f.textures->n_textures > 0)
	{
		const JpTextures* t = f.textures;
		if (t->n_materials != js->n_materials) return JP_ERR_INVALID_ARGUMENT;
		fs.tex_img.resize((size_t)t->n_textures);
		for (int k = 0; k < t->n_textures; k++) if (t->tex_type[k] == JP_TEXTURE_IMAGE) fs.tex_img[k] = load_rgb8(t->texels, t->tex_offset[k], t->tex_width[k], t->tex_height[k]);
	}
	if (f.normal_maps && f.normal_maps->n_maps > 0)
	{
		const JpNormalMaps* m = f.normal_maps;
		if (m->n_materials != js->n_materials) return JP_ERR_INVALID_ARGUMENT;
		for (int k = 0; k < m->n_maps; k++) fs.nmap_img.push_back(load_rgb8(m->texels, m->map_offset[k], m->map_width[k], m->map_height[k]));
	}
	fs.tri_smooth.assign((size_t)std::max(1, js->n_triangles), 0);
	if (f.normals && f.normals->tri_vn)
	{
		if (f.normals->n_triangles != js->n_triangles) return JP_ERR_INVALID_ARGUMENT;
		for (int i = 0; i < js->n_triangles; i++) fs.tri_smooth[i] = jp_vertex_normals_class(f.normals->tri_vn + 9 * (size_t)i) == 1;
	}
	fs.lens_on = false;
	if (f.lens && f.lens->radius > 0.f)
	{
		if (jp_lens_check(f.lens) != 0 || jp_lens_make_plan(&js->camera, f.lens, &fs.lens) != 0) return JP_ERR_INVALID_ARGUMENT;
		fs.lens_on = true;
	}
	fs.film_on = f.film && (f.film->hdr != 0 || f.film->sample_clamp != 0.f);
	if (fs.film_on && jp_film_check(f.film) != 0) return JP_ERR_INVALID_ARGUMENT;
	// sections 18, 19.  A pyramid exists for a texture whose mode is TRILINEAR and that a material uses; a record counts where a material uses its texture.
	const JpTextures* T = (f.textures && f.textures->n_textures > 0) ? f.textures : nullptr;
	const int nt = T ? T->n_textures : 0;
	std::vector<char> used((size_t)nt, 0);
	if (T) for (int m = 0; m < T->n_materials; m++) { const int k = T->mat_texture[m]; if (k >= 0 && k < nt) used[k] = 1; }
	fs.pyr.assign((size_t)nt, Pyramid());
	JpProcDev none; std::memset(&none, 0, sizeof(none));
	fs.proc.assign((size_t)nt, none);
	bool any_pyramid = false, any_antialiased = false;
	if (f.mipmaps)
	{
		const JpTextureMipmaps* M = f.mipmaps;
		int bad, n_on;
		if (jp_mipmaps_check(M, &bad, &n_on) != 0 || M->n_textures != nt) return JP_ERR_INVALID_ARGUMENT;
		for (int t = 0; M->mode && t < nt; t++)
		{
			if (M->mode[t] != JP_MIP_TRILINEAR) continue;
			if (T->tex_type[t] != JP_TEXTURE_IMAGE) return JP_ERR_INVALID_ARGUMENT;          // mipmaps on a solid or checker texture: refused at the upload
			if (!used[t]) continue;
			if (!f.mip_chains || t >= f.n_mip_chains) return JP_ERR_INVALID_ARGUMENT;
			const JpOracleMipChain& c = f.mip_chains[t];
			int w = T->tex_width[t], h = T->tex_height[t], levels = 1;
			for (int m = w > h ? w : h; m > 1; m >>= 1) levels++;                              // L = 1 + floor(log2(max(w, h)))
			if (c.n_levels != levels || !c.level_w || !c.level_h || !c.rgb8) return JP_ERR_INVALID_ARGUMENT;
			Pyramid& P = fs.pyr[t];
			size_t at = 0;
			for (int k = 0; k < levels; k++)
			{
				if (c.level_w[k] != w || c.level_h[k] != h) return JP_ERR_INVALID_ARGUMENT;      // level k + 1: max(1, w_k >> 1) x max(1, h_k >> 1)
				const JpMipLevel l = { w, h, (int32_t)at, 0 }; P.lev.push_back(l);
				at += (size_t)w * h; w = std::max(1, w >> 1); h = std::max(1, h >> 1);
			}
			P.px = load_rgb8(c.rgb8, 0, (int)at, 1).px;
			for (size_t k = 0; k < (size_t)T->tex_width[t] * T->tex_height[t]; k++) if (P.px[k] != fs.tex_img[t].px[k]) return JP_ERR_INVALID_ARGUMENT;   // level 0 is the image
			any_pyramid = true;
		}
	}
	if (f.procedurals && f.procedurals->rec)
	{
		if (f.procedurals->n_textures != nt) return JP_ERR_INVALID_ARGUMENT;
		for (int t = 0; t < nt; t++)
		{
			const JpProcedural& r = f.procedurals->rec[t];
			if (jp_procedural_check(&r) != 0) return JP_ERR_INVALID_ARGUMENT;
			if (r.kind == JP_PROC_NONE) continue;
			if (T->tex_type[t] != JP_TEXTURE_CHECKER) return JP_ERR_INVALID_ARGUMENT;
			for (int k = 0; k < 6; k++) { const float c = T->tex_color[6 * (size_t)t + k]; if (!(c >= 0.f && c <= 1.f)) return JP_ERR_INVALID_ARGUMENT; }
			if (r.space == JP_PROC_SPACE_UV && T->n_triangles > 0 && !T->tri_uv) return JP_ERR_INVALID_ARGUMENT;
			if (!used[t]) continue;
			fs.proc[t] = resolve_record(r);
			if (r.antialias >= 0) any_antialiased = true;
		}
	}
	fs.cone = any_pyramid || any_antialiased;
	fs.footprint_scale = (f.mipmaps && f.mipmaps->footprint_scale != 0.f) ? f.mipmaps->footprint_scale : 1.f;
	fs.bounce_spread = (f.mipmaps && f.mipmaps->bounce_spread != 0.f) ? f.mipmaps->bounce_spread : 0.125f;
	const float* up = js->camera.up;
	fs.gamma0 = 2.f * std::sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]) / js->camera.res_y;
	return JP_OK;
}

// what a path reports besides its radiance
struct PathOut { bool undecided; bool log; JpOracleBranchStats* stats; };
#define PLOG(po, ...) do { if ((po).log) std::printf(__VA_ARGS__); } while (0)

// ---------------------------------------------------------------------------------------------
// section 9: the pick
// ---------------------------------------------------------------------------------------------
inline int light_pick(const JpOracleFeatures& f, float u0, float u1, float& pmf)
{
	int i = (int)(u0 * (float)f.n_lights); if (i > f.n_lights - 1) i = f.n_lights - 1;
	const int j = u1 < f.q[i] ? i : f.alias[i];
	pmf = f.pmf[j];
	return j;
}

// ---------------------------------------------------------------------------------------------
// section 10: the map
// ---------------------------------------------------------------------------------------------
inline V3 to_map(const FState& fs, V3 d) { return fs.f.env_up == JP_ENV_UP_Y ? mk(d.z, d.x, d.y) : d; }       // map (x, y, z) = world (z, x, y)
inline V3 to_world_from_map(const FState& fs, V3 m) { return fs.f.env_up == JP_ENV_UP_Y ? mk(m.y, m.z, m.x) : m; }

inline int env_lookup(const FState& fs, V3 d, PathOut& po)
{
	const int W = fs.f.env_w, H = fs.f.env_h;
	const V3 m = to_map(fs, d);
	const float theta = std::acos(clampf(m.z, -1.f, 1.f));
	float phi = std::atan2(m.y, m.x); if (phi < 0.f) phi += k2Pi;
	const float fr = theta * fs.row_scale, fc = phi * fs.col_scale;
	int row = (int)fr, col = (int)fc;
	if (row > H - 1) row = H - 1;
	if (col > W - 1) col = W - 1;
	if (row < 0) row = 0;
	if (col < 0) col = 0;
	if (near_border(fr, H) || near_border(fc, W)) { po.undecided = true; PLOG(po, "      [undecided map lookup: row coordinate %.9g, column coordinate %.9g]\n", fr, fc); }
	return row * W + col;
}

inline int env_sample(const FState& fs, float a0, float a1, float a2, float b0, float b1, V3& wi, V3& Li, float& pdf)
{
	const int W = fs.f.env_w, H = fs.f.env_h;
	int r0 = (int)(a0 * (float)H), c0 = (int)(a1 * (float)W);
	if (r0 > H - 1) r0 = H - 1;
	if (c0 > W - 1) c0 = W - 1;
	const int i = r0 * W + c0;
	const int j = a2 < fs.f.env_q[i] ? i : fs.f.env_alias[i];
	const int r = j / W, c = j % W;
	const float ct = fs.f.env_row_cos[2 * r], cb = fs.f.env_row_cos[2 * r + 1];
	const float dc = ct - cb;
	const float cosT = ct - b1 * dc;
	// sin^2 = (1 - cos)(1 + cos), the small factor from the row's edge, the other one as 2 minus it ("Sample")
	float s2;
	if (cosT >= 0.f) { const float omc = (1 - ct) + b1 * dc; s2 = omc * (2 - omc); }
	else { const float opc = (1 + cb) + (1 - b1) * dc; s2 = opc * (2 - opc); }
	const float sinT = std::sqrt(smax(0.f, s2));
	const float phi = ((float)c + b0) * fs.phi_step;
	const float sinP = std::sin(phi), cosP = std::cos(phi);
	wi = to_world_from_map(fs, mk(sinT * cosP, sinT * sinP, cosT));
	const float* t = fs.f.env_texel + 4 * (size_t)j;
	Li = ld3(t); pdf = t[3];
	return j;
}

// ---------------------------------------------------------------------------------------------
// section 11: the strategy pdfs and the power heuristic
// ---------------------------------------------------------------------------------------------
inline float mis_weight(float own, float other) { const float r = other / own; return 1.f / (1.f + r * r); }   // 1 / (1 + (other / own)^2)

// the pdf sample_local reports for wi (local frame) under the chosen closure
inline float pdf_local(const Closure& c, V3 wo, V3 wi)
{
	if (!same_hemi(wo, wi)) return 0.f;
	if (c.kind == CL_LAMBERT) return std::abs(wi.z) * kInvPi;
	if (c.kind != CL_MICROFACET) return 0.f;
	V3 wh = wi + wo;
	if (wh.x == 0 && wh.y == 0 && wh.z == 0) return 0.f;
	wh = normalize(wh);
	return tr_Pdf(c, wo, wh) / (4 * dot(wo, wh));
}

inline bool inside_sphere_light(const Scene& sc, int li, V3 p)
{
	const JpScene* js = sc.js;
	if (js->light_type[li] != JP_LIGHT_AREA) return false;
	const int prim = js->light_prim[li];
	if (js->prim_shape_type[prim] != JP_SHAPE_SPHERE) return false;
	const Sph& S = sc.sphs[js->prim_shape_index[prim]];
	return len2(p - S.c) <= S.r * S.r;
}
// does light li take part in the weighting when sampled from p: delta lights do not, a sphere light whose interior holds p does not
inline bool light_weighed(const Scene& sc, int li, V3 p)
{
	const int lt = sc.js->light_type[li];
	if (lt == JP_LIGHT_ENVIRONMENT) return true;
	if (lt != JP_LIGHT_AREA) return false;
	return !inside_sphere_light(sc, li, p);
}

// a = pmf_li * pdf_Li for "the ray from p along d reached light li after dist" (a miss for the environment lights); 0: cannot be sampled there
inline float light_pdf(const FState& fs, const Scene& sc, int li, V3 p, V3 d, float dist, bool& unweighed, PathOut& po)
{
	const JpScene* js = sc.js;
	unweighed = false;
	float pdf;
	if (fs.has_map && li == fs.f.env_light) pdf = fs.f.env_texel[4 * (size_t)env_lookup(fs, d, po) + 3];
	else
	{
		const int lt = js->light_type[li];
		if (lt == JP_LIGHT_ENVIRONMENT)
		{
			const float sinT = std::sqrt(d.x * d.x + d.y * d.y);
			pdf = 1 / (2 * kPi * kPi * sinT);
		}
		else if (lt != JP_LIGHT_AREA) return 0.f;
		else
		{
			const int prim = js->light_prim[li];
			const int type = js->prim_shape_type[prim], i = js->prim_shape_index[prim];
			if (type != JP_SHAPE_SPHERE)
			{
				const V3 ln = type == JP_SHAPE_TRIANGLE ? sc.tris[i].n : (type == JP_SHAPE_RECTANGLE ? sc.rects[i].n : sc.disks[i].n);
				const float inv_area = 1 / shape_area(sc, prim);
				pdf = inv_area * ((dist * dist) / absdot(ln, -d));
			}
			else
			{
				const Sph& S = sc.sphs[i];
				if (len2(p - S.c) <= S.r * S.r) { unweighed = true; return 0.f; }
				const float sin_max = S.r * (1 / len(p - S.c));
				const float cos_max = std::sqrt(smax(0.f, 1 - sin_max * sin_max));
				pdf = 1 / (2 * kPi * (1 - cos_max));
			}
		}
	}
	const float a = fs.f.pmf[li] * pdf;
	return (a > 0.f && !std::isinf(a)) ? a : 0.f;
}

// ---------------------------------------------------------------------------------------------
// section 7: uv of each shape, texture lookups.  libm: the uv came through atan2f / asinf (sphere, disk)
// ---------------------------------------------------------------------------------------------
inline void shape_uv(const Scene& sc, int prim, V3 p, const float* tri_uv, float& u, float& v, bool& libm)
{
	const JpScene* js = sc.js;
	const int type = js->prim_shape_type[prim], i = js->prim_shape_index[prim];
	u = v = 0.f; libm = false;
	if (type == JP_SHAPE_TRIANGLE)
	{
		if (!tri_uv) return;
		const Tri& T = sc.tris[i];
		const V3 e = T.p1 - T.p0, f = T.p2 - T.p0, g = p - T.p0;
		float b1, b2; jp_barycentrics(e.x, e.y, e.z, f.x, f.y, f.z, g.x, g.y, g.z, &b1, &b2);
		const float b0 = 1.f - b1 - b2;
		const float* t = tri_uv + 6 * (size_t)i;
		u = b0 * t[0] + b1 * t[2] + b2 * t[4];
		v = b0 * t[1] + b1 * t[3] + b2 * t[5];
	}
	else if (type == JP_SHAPE_RECTANGLE)                                      // FRectangle::GetUV
	{
		const Rect& R = sc.rects[i];
		const V3 v01 = R.p1 - R.p0, v03 = R.p3 - R.p0, v0p = p - R.p0;
		u = dot(v01, v0p) / len2(v01);
		v = dot(v03, v0p) / len2(v03);
	}
	else if (type == JP_SHAPE_DISK)                                           // FDisk::GetUV in FFrame(normal)
	{
		const Disk& D = sc.disks[i];
		const Frame fr = frame_from_z(D.n);
		const V3 v0 = p - D.c, v1 = to_local(fr, v0);
		float phi = std::atan2(v1.y, v1.x);
		if (phi < 0) phi += k2Pi;
		u = phi / k2Pi;
		v = len(v0) / D.r;
		libm = true;
	}
	else                                                                       // FSphere::GetUV on (p - center) / radius
	{
		const Sph& S = sc.sphs[i];
		const V3 d = (p - S.c) / S.r;
		const float phi = std::atan2(d.z, d.x);
		const float theta = std::asin(std::fmin(std::fmax(d.y, -1.f), 1.f));
		u = 1 - (phi + kPi) / k2Pi;
		v = (theta + kPiOver2) / kPi;
		libm = true;
	}
}

// ---------------------------------------------------------------------------------------------
// section 18: the cone of a path, the footprint of the cone at a hit
// ---------------------------------------------------------------------------------------------
struct Cone { float width, spread; };

// the step at a hit at distance t of the segment the path is on: `bounce` is the number of scattering events behind the segment (a null-material primitive
// does not count), `specular` the flag of the BSDF sample that made the last of them
inline void cone_step(const FState& fs, int bounce, bool specular, float t, Cone& c)
{
	if (bounce == 0) { c.spread = fs.gamma0; c.width = c.spread * t; return; }      // whatever the cone held: after a null-material primitive at bounce 0 it starts again
	if (!specular) c.spread = c.spread > fs.bounce_spread ? c.spread : fs.bounce_spread;
	c.width = c.width + c.spread * t;
}

inline float cross_len(V3 a, V3 b)
{
	const float x = a.y * b.z - a.z * b.y, y = a.z * b.x - a.x * b.z, z = a.x * b.y - a.y * b.x;
	return std::sqrt((x * x + y * y) + z * z);
}
// A = |dpdu x dpdv|, the world area per unit of uv area at p; 0: none (a triangle without a uv set or with a degenerate one, a pole, a disk's centre)
inline float footprint_area(const Scene& sc, int prim, V3 p, const float* tri_uv)
{
	const JpScene* js = sc.js;
	const int type = js->prim_shape_type[prim], i = js->prim_shape_index[prim];
	if (type == JP_SHAPE_TRIANGLE)
	{
		if (!tri_uv) return 0.f;
		const Tri& T = sc.tris[i];
		const float* t = tri_uv + 6 * (size_t)i;
		const float du1 = t[2] - t[0], dv1 = t[3] - t[1], du2 = t[4] - t[0], dv2 = t[5] - t[1];
		const float det = du1 * dv2 - dv1 * du2;
		if (det == 0.f || !(det - det == 0.f)) return 0.f;
		return cross_len(T.p1 - T.p0, T.p2 - T.p0) / std::fabs(det);
	}
	if (type == JP_SHAPE_RECTANGLE) { const Rect& R = sc.rects[i]; return cross_len(R.p1 - R.p0, R.p3 - R.p0); }
	if (type == JP_SHAPE_DISK) { const Disk& D = sc.disks[i]; const V3 v = p - D.c; return (6.2831855f * D.r) * std::sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }
	const Sph& S = sc.sphs[i];
	const V3 d = p - S.c;
	return (19.739209f * S.r) * std::sqrt(d.x * d.x + d.z * d.z);                   // 2 pi^2 r sqrt(d.x^2 + d.z^2)
}
// rho in texels of level 0; su, sv: the active record's uv scale, 1 without one
inline float footprint_rho(float width, float A, int w, int h, float su, float sv, float footprint_scale)
{
	if (!(A > 0.f) || !(A - A == 0.f)) return 0.f;
	const float rho = width * std::sqrt((((float)w * su) * ((float)h * sv)) / A) * footprint_scale;
	return rho - rho == 0.f ? rho : 0.f;
}

// section 19: which octaves a lookup of footprint fw evaluates (k_i = fw 2^i; a_i = 1 for k_i <= 0.25, 0 for k_i >= 0.5, else (0.5 - k_i) 4) -- for the branch
// statistics and the debug print; the value itself is jp_proc_lookup's
inline void octave_classes(float fw, int octaves, bool& all_one, bool& partial, bool& early, PathOut& po)
{
	all_one = true; partial = early = false;
	float k = fw;
	for (int i = 0; i < octaves; i++)
	{
		const float a = k <= 0.25f ? 1.f : (k >= 0.5f ? 0.f : (0.5f - k) * 4.f);
		PLOG(po, " a_%d = %.9g", i, a);
		if (a == 0.f) { early = true; all_one = false; break; }
		if (a < 1.f) { partial = true; all_one = false; }
		k = k * 2.f;
	}
}

inline V3 word_rgb(unsigned int w)
{
	const float s = 1.0f / 255.0f;
	return mk(s * (float)(w & 0xffu), s * (float)((w >> 8) & 0xffu), s * (float)((w >> 16) & 0xffu));
}

// the colour of the textured slot at the hit; false: the material carries no texture.  width: the cone's width at the hit (0: the paths carry none); bounce: of the segment
inline bool textured_color(const FState& fs, const Scene& sc, const Isect& is, float width, int bounce, V3& kd, PathOut& po)
{
	const JpTextures* T = fs.f.textures;
	if (!T || T->n_textures <= 0) return false;
	const int mat = sc.js->prim_material[is.prim];
	if (mat < 0) return false;
	const int t = T->mat_texture[mat];
	if (t < 0) return false;
	const float* col = T->tex_color + 6 * (size_t)t;
	const int b1 = bounce > 0 ? 1 : 0;
	if (T->tex_type[t] == JP_TEXTURE_SOLID) { kd = ld3(col); return true; }
	if (T->tex_type[t] == JP_TEXTURE_CHECKER && fs.proc[t].kind != JP_PROC_NONE)
	{   // section 19: a record takes the plain checker's place, between its two colours
		const JpProcDev& r = fs.proc[t];
		float u = 0.f, v = 0.f; bool libm = false;
		if (r.space == JP_PROC_SPACE_UV) shape_uv(sc, is.prim, is.p, T->tri_uv, u, v, libm);
		if (libm) { po.undecided = true; PLOG(po, "      [undecided: a uv-space procedural on a sphere or disk uv]\n"); }   // every coordinate matters
		const float pp[3] = { is.p.x, is.p.y, is.p.z }, c_odd[3] = { col[0], col[1], col[2] }, c_even[3] = { col[3], col[4], col[5] };
		float tt;
		const unsigned int w = jp_proc_lookup(&r, c_even, c_odd, t, pp, u, v, width, &tt);
		float fw = width * r.s; if (!(fw > 0.f)) fw = 0.f;
		PLOG(po, "    procedural kind %d on texture %d: width %.9g, fw %.9g, t %.9g, word %08x;", r.kind, t, width, fw, tt, w);
		if (r.kind == JP_PROC_CHECKER_AA)
		{
			const bool plain = (w & JP_PROC_TAG_COLOR) != 0 && (w & JP_PROC_TAG_IMAGE) == 0;
			float q[3]; jp_proc_point(&r, pp, u, v, q);
			const bool half = !plain && (!jp_proc_in_range(q[0]) || !jp_proc_in_range(q[1]) || !jp_proc_in_range(q[2]) || !(fw * JP_PROC_10_OVER_PI < JP_PROC_CHECKER_MAX));
			PLOG(po, " fy %.9g: %s\n", fw * JP_PROC_10_OVER_PI, plain ? "the plain checker's word" : (half ? "exactly 0.5" : "filtered"));
			if (po.stats) { if (plain) po.stats->checker_plain[b1]++; else if (half) po.stats->checker_half[b1]++; else po.stats->checker_filtered[b1]++; }
		}
		else
		{
			bool all_one, partial, early; octave_classes(fw, r.octaves, all_one, partial, early, po);
			PLOG(po, "\n");
			if (po.stats) { if (all_one) po.stats->proc_all_one[r.kind][b1]++; if (partial) po.stats->proc_partial[r.kind][b1]++; if (early) po.stats->proc_early[r.kind][b1]++; }
		}
		if (po.stats) po.stats->word_sum[b1] += w;
		// the word: the colour's RGB8 under the image tag, or -- the plain checker's own word -- an entry of the colour table, 2 texture + parity: odd [0..2], even [3..5]
		if (w & JP_PROC_TAG_IMAGE) kd = word_rgb(w);
		else kd = ((w & 0x3fffffffu) - 2u * (unsigned int)t) == 0u ? ld3(col) : ld3(col + 3);
		return true;
	}
	if (T->tex_type[t] == JP_TEXTURE_CHECKER)
	{
		const float sx = std::sin(10 * is.p.x), sy = std::sin(10 * is.p.y), sz = std::sin(10 * is.p.z);
		kd = (sx * sy * sz < 0.0f) ? ld3(col) : ld3(col + 3);
		return true;
	}
	const Image& im = fs.tex_img[t];
	float u, v; bool libm; shape_uv(sc, is.prim, is.p, T->tri_uv, u, v, libm);
	unsigned int w;
	const JpTexSampler* rec = fs.tex_rec(t);
	const Pyramid& P = fs.pyr[t];
	float rho = 0.f;
	if (!P.lev.empty())
	{   // section 18: the footprint in texels; above one texel the trilinear lookup, else the lookup the texture has without mipmaps
		const float A = footprint_area(sc, is.prim, is.p, T->tri_uv);
		rho = footprint_rho(width, A, im.w, im.h, rec ? rec->scale_u : 1.f, rec ? rec->scale_v : 1.f, fs.footprint_scale);
		PLOG(po, "    mip on texture %d: width %.9g, A %.9g, rho %.9g", t, width, A, rho);
		if (po.stats) { if (rho == 0.f) po.stats->mip_rho_zero[b1]++; else if (rho <= 1.f) po.stats->mip_rho_le1[b1]++; }
	}
	if (rho > 1.f)
	{
		const int levels = (int)P.lev.size();
		const int l = jp_mip_level_of(rho);
		const JpTexSampler ident = jp_mip_identity_sampler();                  // a texture without an active record is addressed through the identity record here
		w = jp_mip_lookup_above(rec ? rec : &ident, P.px.data(), P.lev.data(), levels, u, v, rho);
		if (l >= levels - 1) { PLOG(po, ", l %d: level %d alone", l, levels - 1); if (po.stats) po.stats->mip_last_level[b1]++; }
		else { PLOG(po, ", l %d, f %.9g", l, jp_mip_fraction(rho, l)); if (po.stats) po.stats->mip_two_level[b1][l < 15 ? l : 15]++; }
		if (libm) { po.undecided = true; PLOG(po, " [undecided: a trilinear lookup on a sphere or disk uv]"); }   // bilinear weights on two levels: every coordinate matters
	}
	else if (rec)
	{
		w = jp_tex_lookup_sampled(rec, im.px.data(), im.w, im.h, u, v);
		if (libm) { po.undecided = true; PLOG(po, "      [undecided: a texture under a sampling record on a sphere or disk uv]\n"); }   // wraps and bilinear weights: every coordinate matters
	}
	else
	{   // FImageTexture::Sample: clamp, flip v, nearest texel
		const float uc = u < 0.f ? 0.f : (u > 1.f ? 1.f : u);
		const float vc = 1.f - (v < 0.f ? 0.f : (v > 1.f ? 1.f : v));
		const float fi = uc * (float)im.w, fj = vc * (float)im.h;
		int i = fi >= 0.f ? (int)fi : 0, j = fj >= 0.f ? (int)fj : 0;
		if (i >= im.w) i = im.w - 1;
		if (j >= im.h) j = im.h - 1;
		w = im.px[(size_t)j * im.w + i];
		if (libm && (near_border(fi, im.w) || near_border(fj, im.h))) { po.undecided = true; PLOG(po, "      [undecided image lookup: texel coordinates %.9g, %.9g]\n", fi, fj); }
	}
	if (!P.lev.empty()) { PLOG(po, ", texel %06x\n", w & 0xffffffu); if (po.stats) po.stats->word_sum[b1] += w & 0xffffffu; }
	kd = word_rgb(w);
	return true;
}

// FMaterial::Scattering with the textured slot [0..2] taken from kd: matte diffuseColor, mirror specularColor, plastic Kd with Qd recomputed from it
inline bool scattering_textured(const JpScene* js, int mat, V3 normal, V3 kd, Draw& rnd, Closure& c)
{
	const float* p = js->mat_params + (size_t)mat * JP_MAT_PARAM_STRIDE;
	const int type = js->mat_type[mat];
	c.c0 = c.c1 = splat(0); c.eta_i = c.eta_t = 1; c.ax = c.ay = 0; c.fresnel = FR_CONDUCTOR; c.feta = c.fk = splat(0);
	float up = 0.f;
	if (type == JP_MAT_PLASTIC) up = rnd.get1();
	c.frame = frame_from_z(normal);
	if (type == JP_MAT_MATTE) { c.kind = CL_LAMBERT; c.c0 = kd; return true; }
	if (type == JP_MAT_MIRROR) { c.kind = CL_MIRROR; c.c0 = kd; return true; }
	if (type != JP_MAT_PLASTIC) return false;                                 // (glass, metal: refused at upload)
	const V3 ks = ld3(p + 3);
	const float Ld = 0.212671f * kd.x + 0.715160f * kd.y + 0.072169f * kd.z;     // FColor::Luminance, left to right
	const float Ls = 0.212671f * ks.x + 0.715160f * ks.y + 0.072169f * ks.z;
	const float Qd = Ld / (Ld + Ls);
	if (up < Qd) { c.kind = CL_LAMBERT; c.c0 = kd / Qd; }
	else { c.kind = CL_MICROFACET; c.c0 = ks / (1 - Qd); c.fresnel = FR_DIELECTRIC; c.ax = c.ay = smax(0.001f, p[6]); }
	return true;
}

// ---------------------------------------------------------------------------------------------
// sections 12, 14: the shading normal.  on: the hit has one of its own (a smooth triangle, a map that perturbs it)
// ---------------------------------------------------------------------------------------------
inline V3 shading_normal(const FState& fs, const Scene& sc, const Isect& is, bool& on, PathOut& po)
{
	const JpScene* js = sc.js;
	const V3 N = is.n;
	V3 Ns = N; on = false;
	const int type = js->prim_shape_type[is.prim], i = js->prim_shape_index[is.prim];
	if (type == JP_SHAPE_TRIANGLE && fs.tri_smooth[i])
	{
		const Tri& T = sc.tris[i];
		const float p0[3] = { T.p0.x, T.p0.y, T.p0.z }, p1[3] = { T.p1.x, T.p1.y, T.p1.z }, p2[3] = { T.p2.x, T.p2.y, T.p2.z }, ng[3] = { T.n.x, T.n.y, T.n.z }, p[3] = { is.p.x, is.p.y, is.p.z };
		float ns[3]; jp_shading_normal_at(p0, p1, p2, ng, fs.f.normals->tri_vn + 9 * (size_t)i, p, ns);
		Ns = mk(ns[0], ns[1], ns[2]); on = true;
	}
	const JpNormalMaps* M = fs.f.normal_maps;
	const int mat = js->prim_material[is.prim];
	if (!M || M->n_maps <= 0 || mat < 0) return Ns;
	const int k = M->mat_map[mat];
	if (k < 0) return Ns;
	float dpdu[3], dpdv[3];
	if (type == JP_SHAPE_TRIANGLE)
	{
		if (!M->tri_uv) return Ns;
		const Tri& T = sc.tris[i];
		const float p0[3] = { T.p0.x, T.p0.y, T.p0.z }, p1[3] = { T.p1.x, T.p1.y, T.p1.z }, p2[3] = { T.p2.x, T.p2.y, T.p2.z };
		if (!jp_triangle_tangents_at(p0, p1, p2, M->tri_uv + 6 * (size_t)i, dpdu, dpdv)) return Ns;
	}
	else if (type == JP_SHAPE_RECTANGLE)
	{
		const Rect& R = sc.rects[i];
		const V3 a = R.p1 - R.p0, b = R.p3 - R.p0;
		dpdu[0] = a.x; dpdu[1] = a.y; dpdu[2] = a.z; dpdv[0] = b.x; dpdv[1] = b.y; dpdv[2] = b.z;
	}
	else if (type == JP_SHAPE_DISK)
	{
		const Disk& D = sc.disks[i];
		const Frame fr = frame_from_z(D.n);
		const V3 v0 = is.p - D.c;
		const float s[3] = { fr.s.x, fr.s.y, fr.s.z }, t[3] = { fr.t.x, fr.t.y, fr.t.z }, v[3] = { v0.x, v0.y, v0.z };
		jp_disk_tangents_at(s, t, v, dpdu, dpdv);
	}
	else
	{
		const V3 d = is.p - sc.sphs[i].c;
		const float dd[3] = { d.x, d.y, d.z };
		jp_sphere_tangents_at(dd, dpdu, dpdv);
	}
	float u, v; bool libm; shape_uv(sc, is.prim, is.p, M->tri_uv, u, v, libm);
	const Image& im = fs.nmap_img[k];
	const float strength = M->mat_strength ? M->mat_strength[mat] : 1.f;
	// the bilinear weights move with every ulp of the angle -- unless nothing can come of them: strength 0, or a map whose R and G are 128 everywhere (x = y = 0 exactly)
	bool neutral = strength == 0.f;
	if (!neutral) { neutral = true; for (unsigned int t : im.px) if ((t & 0xffffu) != 0x8080u) { neutral = false; break; } }
	if (libm && !neutral) { po.undecided = true; PLOG(po, "      [undecided: a bilinear normal-map lookup on a sphere or disk uv]\n"); }
	const float nb[3] = { Ns.x, Ns.y, Ns.z }, ng[3] = { N.x, N.y, N.z };
	float ns[3];
	if (jp_perturb_normal_sampled(fs.map_rec(k), nb, ng, dpdu, dpdv, u, v, im.px.data(), im.w, im.h, strength, ns)) { Ns = mk(ns[0], ns[1], ns[2]); on = true; }
	return Ns;
}

// ---------------------------------------------------------------------------------------------
// the path: FPathIntegratorIteration::Li (pt_oracle.cc Li) with the features of sections 7 and 9 - 16
// ---------------------------------------------------------------------------------------------
V3 LiFeatures(const FState& fs, const Scene& sc, const Ray& inRay, Draw& rnd, int maxDepth, Counts& cn, PathOut& po)
{
	const JpScene* js = sc.js;
	const JpOracleFeatures& f = fs.f;
	V3 L = mk(0, 0, 0), beta = mk(1, 1, 1);
	Ray ray = inRay;
	bool specular = false;
	Cone cone = { 0.f, 0.f };                         // section 18
	float carried_pdf = 0.f, carried_dist = 0.f;      // section 11 "Carried state": the pdf the BSDF sample that produced the ray was drawn with, the distance since that shading point
	for (int bounces = 0;; ++bounces)
	{
		Isect is; is.prim = -1;
		const bool found = sc.intersect(ray, is);
		const float t_hit = ray.tmax;
		cn.closest++; if (found) cn.closest_hit++;
		const bool direct = bounces == 0 || specular;  // emission counts in full
		PLOG(po, "  bounce %d%s: origin (%.9g %.9g %.9g) dir (%.9g %.9g %.9g) -> %s", bounces, specular ? " (after a specular bounce)" : "", ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, found ? "hit" : "miss\n");
		if (found) PLOG(po, " primitive %d at t %.9g, p (%.9g %.9g %.9g), N (%.9g %.9g %.9g)\n", is.prim, t_hit, is.p.x, is.p.y, is.p.z, is.n.x, is.n.y, is.n.z);
		if (found)
		{
			const int li = js->prim_light[is.prim];
			if (li >= 0 && dot(is.n, is.wo) > 0.f)
			{
				const V3 Le = ld3(js->light_radiance + 3 * li);
				if (!isblack(Le))
				{
					float w = 1.f;
					bool counts = direct;
					if (!direct && fs.mis)
					{   // the BSDF sample of the last shading event reached an emitter: weighed against the light strategy's pdf, taken from that shading point
						bool unweighed;
						const float a = light_pdf(fs, sc, li, ray.o - carried_dist * ray.d, ray.d, carried_dist + t_hit, unweighed, po);
						w = unweighed ? 0.f : (a > 0.f ? mis_weight(carried_pdf, a) : 1.f);
						counts = true;
						PLOG(po, "    emitter hit (light %d): a = %.9g, b = %.9g, weight %.9g\n", li, a, carried_pdf, w);
					}
					if (counts) { L = L + (fs.mis ? cmul(beta, Le) * w : cmul(beta, Le)); PLOG(po, "    emission -> L (%.9g %.9g %.9g)\n", L.x, L.y, L.z); }
				}
			}
		}
		else if (direct)
		{
			if (fs.has_map) L = L + cmul(beta, ld3(f.env_texel + 4 * (size_t)env_lookup(fs, ray.d, po)));
			else if (fs.pick) for (int e = 0; e < f.n_env; e++) L = L + cmul(beta, ld3(js->light_radiance + 3 * f.env_lights[e]));
			else for (size_t k = 0; k < sc.infiniteLights.size(); k++) L = L + cmul(beta, ld3(js->light_radiance + 3 * sc.infiniteLights[k]));
			PLOG(po, "    environment -> L (%.9g %.9g %.9g)\n", L.x, L.y, L.z);
		}
		else if (fs.mis)
		{   // the BSDF sample left the scene: every environment light it sees is a strategy of its own, in light order
			const int ne = fs.has_map ? 1 : f.n_env;
			for (int e = 0; e < ne; e++)
			{
				int l2; V3 Lr;
				if (fs.has_map) { l2 = f.env_light; Lr = ld3(f.env_texel + 4 * (size_t)env_lookup(fs, ray.d, po)); }
				else { l2 = f.env_lights[e]; Lr = ld3(js->light_radiance + 3 * l2); }
				bool unweighed;
				const float a = light_pdf(fs, sc, l2, ray.o, ray.d, 0.f, unweighed, po);
				const float w = a > 0.f ? mis_weight(carried_pdf, a) : 1.f;
				L = L + cmul(beta, Lr) * w;
				PLOG(po, "    miss, environment light %d: a = %.9g, b = %.9g, weight %.9g -> L (%.9g %.9g %.9g)\n", l2, a, carried_pdf, w, L.x, L.y, L.z);
			}
		}
		if (found)
		{   // section 18: the cone is stepped at every hit -- textured, untextured or without a material -- with the flag of the BSDF sample that made the segment
			cone_step(fs, bounces, specular, t_hit, cone);
			if (fs.cone) PLOG(po, "    cone: width %.9g, spread %.9g\n", cone.width, cone.spread);
		}
		if (!found || bounces >= maxDepth) break;
		const int mat = js->prim_material[is.prim];
		if (mat < 0)
		{   // null material: the path passes through, same bounce (and the same specular flag), the carried record goes along
			carried_dist = carried_dist + t_hit;
			ray = mkray(is.p, ray.d);
			--bounces;
			PLOG(po, "    null material: pass through (carried distance %.9g)\n", carried_dist);
			continue;
		}
		const V3 N = is.n;                              // geometric: emission, light sampling, pdfs, the guard
		bool own_normal;
		const V3 Ns = shading_normal(fs, sc, is, own_normal, po);   // the frame and both cosines
		const bool guard = own_normal && js->mat_type[mat] != JP_MAT_GLASS;
		if (own_normal) PLOG(po, "    Ns (%.9g %.9g %.9g)%s\n", Ns.x, Ns.y, Ns.z, guard ? ", guarded" : "");
		Closure c;
		V3 kd;
		const unsigned dim0 = rnd.s ? rnd.s->dim : 0u;
		if (textured_color(fs, sc, is, fs.cone ? cone.width : 0.f, bounces, kd, po)) { PLOG(po, "    texture colour (%.9g %.9g %.9g)\n", kd.x, kd.y, kd.z); scattering_textured(js, mat, Ns, kd, rnd, c); }
		else scattering(js, mat, Ns, rnd, c);
		PLOG(po, "    material %d (type %d), closure kind %d, draws from dim %u\n", mat, js->mat_type[mat], c.kind, dim0);
		if (!c.delta())
		{
			const int nl = fs.pick ? (js->n_lights > 0 ? 1 : 0) : js->n_lights;
			for (int it = 0; it < nl; it++)
			{
				int li = it; float pmf = 1.f;
				if (fs.pick) { float u0, u1; rnd.get2(u0, u1); li = light_pick(f, u0, u1, pmf); PLOG(po, "    pick (%.9g, %.9g) -> light %d, pmf %.9g\n", u0, u1, li, pmf); }
				const bool mapped = fs.has_map && li == f.env_light;
				LightSample ls;
				if (mapped)
				{
					float a0, a1, a2, b0, b1; rnd.get2(a0, a1); a2 = rnd.get1(); rnd.get2(b0, b1);      // five draws, consumed whatever becomes of the sample
					if (!(pmf > 0.f)) continue;
					const int j = env_sample(fs, a0, a1, a2, b0, b1, ls.wi, ls.Li, ls.pdf);
					ls.pos = is.p + ls.wi * 2 * js->world_radius;
					PLOG(po, "    map sample (%.9g %.9g %.9g %.9g %.9g) -> texel %d, wi (%.9g %.9g %.9g), pdf %.9g\n", a0, a1, a2, b0, b1, j, ls.wi.x, ls.wi.y, ls.wi.z, ls.pdf);
				}
				else
				{
					float ux, uy; rnd.get2(ux, uy);                                                      // two draws, consumed whatever becomes of the sample
					if (fs.pick && !(pmf > 0.f)) continue;
					ls = sample_li(sc, li, is, ux, uy);
					PLOG(po, "    light %d sample (%.9g, %.9g): wi (%.9g %.9g %.9g), pdf %.9g, Li (%.9g %.9g %.9g)\n", li, ux, uy, ls.wi.x, ls.wi.y, ls.wi.z, ls.pdf, ls.Li.x, ls.Li.y, ls.Li.z);
				}
				if (isblack(ls.Li) || ls.pdf == 0.f) continue;
				const V3 fv = bsdf_eval(c, is.wo, ls.wi);
				if (isblack(fv)) continue;
				if (guard && dot(ls.wi, N) * dot(is.wo, N) <= 0.f) { PLOG(po, "    refused: the other geometric side\n"); continue; }
				if (occluded(sc, is, ls.pos, cn)) { PLOG(po, "    occluded\n"); continue; }
				V3 contrib = cmul(cmul(beta, fv), ls.Li) * absdot(ls.wi, Ns) / ls.pdf;
				if (fs.pick) contrib = contrib / pmf;
				if (fs.mis && (mapped || light_weighed(sc, li, is.p)))
				{
					const float a = pmf * ls.pdf, b = pdf_local(c, to_local(c.frame, is.wo), to_local(c.frame, ls.wi));
					const float w = mis_weight(a, b);
					contrib = contrib * w;
					PLOG(po, "    light side: a = %.9g, b = %.9g, weight %.9g\n", a, b, w);
				}
				L = L + contrib;
				PLOG(po, "    f (%.9g %.9g %.9g), contribution (%.9g %.9g %.9g) -> L (%.9g %.9g %.9g)\n", fv.x, fv.y, fv.z, contrib.x, contrib.y, contrib.z, L.x, L.y, L.z);
			}
		}
		float ux, uy; rnd.get2(ux, uy);
		const BsdfSample bs = bsdf_sample(c, is.wo, ux, uy);
		PLOG(po, "    BSDF sample (%.9g, %.9g): wi (%.9g %.9g %.9g), f (%.9g %.9g %.9g), pdf %.9g, flags %d\n", ux, uy, bs.wi.x, bs.wi.y, bs.wi.z, bs.f.x, bs.f.y, bs.f.z, bs.pdf, bs.flags);
		if (isblack(bs.f) || bs.pdf == 0.f) break;
		if (guard && dot(bs.wi, N) * dot(is.wo, N) <= 0.f) { PLOG(po, "    refused: the other geometric side; the path ends\n"); break; }
		specular = (bs.flags & BS_SPECULAR) != 0;
		if (bounces >= 3)
		{
			const float q = smax(0.05f, 1 - maxcomp(bs.f));
			const float ur = rnd.get1();
			PLOG(po, "    roulette: q %.9g, draw %.9g\n", q, ur);
			if (ur < q) break;
			beta = cmul(beta, bs.f * absdot(bs.wi, Ns) / (bs.pdf * (1 - q)));
		}
		else beta = cmul(beta, bs.f * absdot(bs.wi, Ns) / bs.pdf);
		ray = mkray(is.p, bs.wi);
		carried_pdf = bs.pdf; carried_dist = 0.f;
		PLOG(po, "    beta (%.9g %.9g %.9g)\n", beta.x, beta.y, beta.z);
	}
	return L;
}

// one camera sample: the draws of the film position, the lens draws (section 13), the path
inline V3 sample_radiance(const FState& fs, const Scene& sc, const JpRenderParams& rp, Sampler& smp, int x, int y, Counts& cn, PathOut& po)
{
	Draw rnd = { &smp, nullptr };
	float fx, fy; smp.camera_sample((float)x, (float)y, fx, fy);
	Ray ray;
	if (fs.lens_on)
	{
		float u0, u1; smp.get2(u0, u1);
		float o[3], d[3]; jp_lens_ray(&sc.js->camera, &fs.lens, fx, fy, u0, u1, o, d);
		ray = mkray(ld3(o), ld3(d));
		PLOG(po, "  lens draws (%.9g, %.9g)\n", u0, u1);
	}
	else ray = camera_ray(sc.js->camera, fx, fy);
	V3 l = rp.integrator == JP_INTEGRATOR_WHITTED ? LiWhitted(sc, ray, rnd, rp.max_depth, 0, cn)
	     : rp.integrator == JP_INTEGRATOR_DEBUG_NORMAL ? LiDebug(sc, ray, cn) : LiFeatures(fs, sc, ray, rnd, rp.max_depth, cn, po);
	if (fs.film_on && fs.f.film->sample_clamp > 0.f) jp_film_clamp_sample(fs.f.film->sample_clamp, &l.x, &l.y, &l.z);      // section 15: before the sample enters the sum
	return l;
}

void render_rows_features(const FState& fs, const Scene& sc, const JpRenderParams& rp, Sampler& smp, int y0, int y1, float* film, uint8_t* undecided, Counts& cn, JpOracleBranchStats* stats)
{
	const float ratio = (float)1 / rp.spp;
	for (int y = y0; y < y1; y++) for (int x = 0; x < rp.width; x++)
	{
		V3 L = mk(0, 0, 0);
		PathOut po = { false, false, stats };
		smp.start_pixel();
		do
		{
			const V3 l = sample_radiance(fs, sc, rp, smp, x, y, cn, po);
			L = L + l * ratio;
		} while (smp.next_sample());
		float* o = film + 3 * ((size_t)y * rp.width + x);
		if (fs.film_on && fs.f.film->hdr) { o[0] = 0.f + smax(L.x, 0.f); o[1] = 0.f + smax(L.y, 0.f); o[2] = 0.f + smax(L.z, 0.f); }
		else { o[0] = 0.f + clampf(L.x, 0.f, 1.f); o[1] = 0.f + clampf(L.y, 0.f, 1.f); o[2] = 0.f + clampf(L.z, 0.f, 1.f); }
		if (undecided) undecided[(size_t)y * rp.width + x] = po.undecided ? 1 : 0;
	}
}

// the refusals of the library for a feature set (sections 7, 9 - 12, 14): the same status
int refusal(const FState& fs, const JpRenderParams& rp)
{
	if (rp.sampler_mode == JP_SAMPLER_STOCK_MT19937 && (fs.pick || fs.lens_on)) return JP_ERR_UNSUPPORTED;     // the features are defined on the counter stream
	if (rp.integrator != JP_INTEGRATOR_WHITTED) return JP_OK;
	bool smooth = false; for (char s : fs.tri_smooth) smooth |= s != 0;
	if (fs.pick || smooth || (fs.f.textures && fs.f.textures->n_textures > 0) || (fs.f.normal_maps && fs.f.normal_maps->n_maps > 0)) return JP_ERR_UNSUPPORTED;
	return JP_OK;
}

} // namespace

extern "C" {

int jp_oracle_render_features(const JpScene* js, const JpRenderParams* rp, const JpOracleFeatures* feat, int nthreads, float* film, JpCounters* out, uint8_t* undecided)
{
	return jp_oracle_render_features_stats(js, rp, feat, nthreads, film, out, undecided, nullptr);
}

int jp_oracle_render_features_stats(const JpScene* js, const JpRenderParams* rp, const JpOracleFeatures* feat, int nthreads, float* film, JpCounters* out, uint8_t* undecided,
                                    JpOracleBranchStats* stats)
{
	if (!js || !rp || !film) return JP_ERR_INVALID_ARGUMENT;
	FState fs;
	if (const int st = prepare(js, feat, fs); st != JP_OK) return st;
	if (const int st = refusal(fs, *rp); st != JP_OK) return st;
	g_watertight = fs.f.watertight != 0;
	Scene sc(js);
	const int W = rp->width, H = rp->height;
	std::memset(film, 0, sizeof(float) * 3 * (size_t)W * H);
	if (undecided) std::memset(undecided, 0, (size_t)W * H);
	Counts total = { 0, 0, 0, 0 };
	const int rows = rp->band_rows > 0 ? rp->band_rows : 20;
	const int nbands = (H + rows - 1) / rows;
	unsigned long long bands_done = 0;
	JpOracleBranchStats sum; std::memset(&sum, 0, sizeof(sum));
	if (nthreads < 1)
	{
		Sampler smp(rp->sampler_mode, rp->seed, rp->spp);
		render_rows_features(fs, sc, *rp, smp, 0, H, film, undecided, total, stats ? &sum : nullptr);
		bands_done = (unsigned long long)H;
	}
	else
	{
		std::atomic<int> next(0);
		std::vector<Counts> per(nthreads, total);
		std::vector<JpOracleBranchStats> per_stats(nthreads, sum);
		std::vector<unsigned long long> rows_done(nthreads, 0);
		std::vector<std::thread> pool;
		for (int t = 0; t < nthreads; t++) pool.push_back(std::thread([&, t]() {
			for (;;)
			{
				const int b = next.fetch_add(1);
				if (b >= nbands) break;
				if (rp->shard_count > 1 && (b % rp->shard_count) != rp->shard_index) continue;
				Sampler smp(rp->sampler_mode, rp->seed, rp->spp);
				int y0 = b * rows, y1 = y0 + rows; if (y1 > H) y1 = H;
				render_rows_features(fs, sc, *rp, smp, y0, y1, film, undecided, per[t], stats ? &per_stats[t] : nullptr);
				rows_done[t] += (unsigned long long)(y1 - y0);
			}
		}));
		for (size_t t = 0; t < pool.size(); t++) pool[t].join();
		for (int t = 0; t < nthreads; t++) { total.closest += per[t].closest; total.closest_hit += per[t].closest_hit; total.shadow += per[t].shadow; total.shadow_occ += per[t].shadow_occ; bands_done += rows_done[t]; }
		for (int t = 0; t < nthreads; t++)
		{   // every field after the header is a uint64_t count
			const uint64_t* a = per_stats[t].mip_rho_zero; uint64_t* b = sum.mip_rho_zero;
			for (size_t k = 0; k < (sizeof(sum) - offsetof(JpOracleBranchStats, mip_rho_zero)) / sizeof(uint64_t); k++) b[k] += a[k];
		}
	}
	g_watertight = false;
	if (stats)
	{
		const int32_t n = std::min((size_t)stats->struct_bytes, sizeof(sum));
		sum.struct_bytes = n; sum.pad = 0;
		if (n >= (int32_t)sizeof(int32_t)) std::memcpy(stats, &sum, (size_t)n);
	}
	if (out)
	{
		std::memset(out, 0, sizeof(*out));
		out->samples = bands_done * (unsigned long long)W * (unsigned long long)rp->spp;
		out->closest_rays = total.closest; out->closest_hits = total.closest_hit; out->shadow_rays = total.shadow; out->shadow_occluded = total.shadow_occ;
	}
	return JP_OK;
}

int jp_oracle_path_features(const JpScene* js, const JpRenderParams* rp, const JpOracleFeatures* feat, int x, int y, int s, float* out_rgb)
{
	if (!js || !rp || x < 0 || y < 0 || s < 0 || x >= rp->width || y >= rp->height || s >= rp->spp) return JP_ERR_INVALID_ARGUMENT;
	FState fs;
	if (const int st = prepare(js, feat, fs); st != JP_OK) return st;
	if (const int st = refusal(fs, *rp); st != JP_OK) return st;
	if (rp->sampler_mode == JP_SAMPLER_STOCK_MT19937) return JP_ERR_UNSUPPORTED;       // one sample alone needs a stream that is addressed, not consumed
	g_watertight = fs.f.watertight != 0;
	Scene sc(js);
	Sampler smp(rp->sampler_mode, rp->seed, rp->spp);
	smp.start_pixel(); smp.sample_index = s;
	Counts cn = { 0, 0, 0, 0 };
	PathOut po = { false, true, nullptr };
	std::printf("pixel (%d, %d) sample %d\n", x, y, s);
	const V3 l = sample_radiance(fs, sc, *rp, smp, x, y, cn, po);
	std::printf("  radiance (%.9g %.9g %.9g)%s; closest rays %llu, hits %llu, shadow rays %llu, occluded %llu\n", l.x, l.y, l.z, po.undecided ? " [undecided]" : "",
	            cn.closest, cn.closest_hit, cn.shadow, cn.shadow_occ);
	std::fflush(stdout);
	g_watertight = false;
	if (out_rgb) { out_rgb[0] = l.x; out_rgb[1] = l.y; out_rgb[2] = l.z; }
	return JP_OK;
}

} // extern "C"
