// jet-pbrt_amd/csrc/jp_tex.h -- texture-mapped materials: the uv of a hit (GetUV of every shape), the texture lookups of texture.cc
// and the closure of a textured material.  k_texel, k_shade_tex and k_surface call these and nothing else (INTEGRATION.md "Textures").
#pragma once
#include "jp_common.h"
#include "jp_normals.h"

namespace jp
{
#define JP_TEX_PI_OVER2 (JP_PI / 2.0f)                                 // kPiOver2 = kPi / 2 (pbrt.h:42)

// uv of the point p on device primitive h (caller's primitive index = meta.x)
__device__ __forceinline__ float2 tex_uv(const float4* prims, const TexView& tv, int h, int prim, V3 p)
{
	const float4 g0 = prims[4 * h], g3 = prims[4 * h + 3];
	const int type = __float_as_int(g3.w);
	float u = 0.f, v = 0.f;
	if (type == JP_SHAPE_TRIANGLE)
	{   // barycentrics by the normal equations (FTriangle::GetUV divides by Dot(p1 - p0, p2 - p0), zero for a right angle at p0)
		if (tv.prim_uv)
		{
			const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
			const V3 e = xyz(g1) - xyz(g0), f = xyz(g2) - xyz(g0), g = p - xyz(g0);
			float b1, b2;
			jp_barycentrics(e.x, e.y, e.z, f.x, f.y, f.z, g.x, g.y, g.z, &b1, &b2);   // (jp_normals.h: the shading normal's barycentrics are these)
			const float b0 = 1.f - b1 - b2;
			const float2 t0 = tv.prim_uv[3 * prim], t1 = tv.prim_uv[3 * prim + 1], t2 = tv.prim_uv[3 * prim + 2];
			u = b0 * t0.x + b1 * t1.x + b2 * t2.x;
			v = b0 * t0.y + b1 * t1.y + b2 * t2.y;
		}
	}
	else if (type == JP_SHAPE_RECTANGLE)                              // FRectangle::GetUV shape.h:437-447; p3 rides in the w components
	{
		const float4 g1 = prims[4 * h + 1], g2 = prims[4 * h + 2];
		const V3 p0 = xyz(g0), v01 = xyz(g1) - p0, v03 = mk(g0.w, g1.w, g2.w) - p0, v0p = p - p0;
		u = dot(v01, v0p) / len2(v01);
		v = dot(v03, v0p) / len2(v03);
	}
	else if (type == JP_SHAPE_DISK)                                   // FDisk::GetUV shape.h:223-235
	{
		const Frame fr = frame_from_z(xyz(prims[4 * h + 1]));
		const V3 v0 = p - xyz(g0), v1 = to_local(fr, v0);
		float phi = atan2f(v1.y, v1.x);
		if (phi < 0) phi += JP_2PI;
		u = phi / JP_2PI;
		v = len(v0) / g0.w;
	}
	else                                                              // FSphere::GetUV shape.h:528-538 on (p - center) / radius
	{
		const V3 d = (p - xyz(g0)) / g0.w;
		const float phi = atan2f(d.z, d.x);
		const float theta = asinf(fminf(fmaxf(d.y, -1.f), 1.f));
		u = 1 - (phi + JP_PI) / JP_2PI;
		v = (theta + JP_TEX_PI_OVER2) / JP_PI;
	}
	return make_float2(u, v);
}

// FTexture::Sample (texture.cc) as a side word: the texel's bytes, or the index of the colour in TexView::col
__device__ __forceinline__ unsigned int tex_sample(const TexView& tv, int t, float2 uv, V3 p)
{
	const int4 d = tv.desc[t];
	if (d.x == JP_TEXTURE_IMAGE)
	{   // FImageTexture::Sample: clamp, flip v, nearest texel; a NaN coordinate selects texel 0 on its axis
		const float u = uv.x < 0.f ? 0.f : (uv.x > 1.f ? 1.f : uv.x);
		const float v = 1.f - (uv.y < 0.f ? 0.f : (uv.y > 1.f ? 1.f : uv.y));
		const float fi = u * (float)d.y, fj = v * (float)d.z;
		int i = fi >= 0.f ? (int)fi : 0, j = fj >= 0.f ? (int)fj : 0;
		if (i >= d.y) i = d.y - 1;
		if (j >= d.z) j = d.z - 1;
		return JP_TEX_IMAGE_TAG | (tv.texels[(size_t)d.w + (size_t)j * (size_t)d.y + (size_t)i] & 0xffffffu);
	}
	unsigned int k = 2u * (unsigned int)t;
	if (d.x == JP_TEXTURE_CHECKER)
	{   // FCheckerTexture::Sample: only the sign of the product matters
		float sx, sy, sz, c;
		sincos_f(10 * p.x, &sx, &c); sincos_f(10 * p.y, &sy, &c); sincos_f(10 * p.z, &sz, &c);
		if (!(sx * sy * sz < 0.0f)) k++;
	}
	return JP_TEX_COLOR_TAG | k;
}

// the colour a side word stands for: (1 / 255) * byte (texture.cc), or a colour of the table
__device__ __forceinline__ V3 tex_color(const TexView& tv, unsigned int w)
{
	// The image tag is the word's sign bit, and w is never 0 here (k_shade_tex tests the word first, tex_sample always tags it): written as the compare
	// `(int)w < 1` the k_shade*_tex kernels have always been built with.  With `w & JP_TEX_IMAGE_TAG` the optimiser picks between that form and
	// `(int)w > -1` depending on what else the translation unit holds, and the two orders of the branches below are different instruction streams
	// (tools/asm_kernel_diff.py; DESIGN.md "Texture sampling").
	if ((int)w < 1)
	{
		const float s = 1.0f / 255.0f;
		return mk(s * (float)(w & 0xffu), s * (float)((w >> 8) & 0xffu), s * (float)((w >> 16) & 0xffu));
	}
	return xyz(tv.col[w & 0x3fffffffu]);
}

// make_closure with the textured slot [0..2] taken from `kd`: matte diffuseColor, mirror specularColor, plastic Kd with its Qd
// recomputed from it as the constructor computes it (material.h:94-98).  Glass and metal are never textured (jp_upload_scene_textured).
template <typename MatPtr>
__device__ __forceinline__ void make_closure_tex(MatPtr mats, int type, int mat, float uplastic, V3 kd, Closure& c)
{
	const float4 p0 = mats[4 * mat + 0], p1 = mats[4 * mat + 1];
	c.c0 = splat(0); c.c1 = splat(0); c.eta_t = 1; c.ax = c.ay = 0; c.fresnel = FR_CONDUCTOR; c.feta = splat(0); c.fk = splat(0);
	if (type == JP_MAT_MATTE) { c.kind = CL_LAMBERT; c.c0 = kd; }
	else if (type == JP_MAT_MIRROR) { c.kind = CL_MIRROR; c.c0 = kd; }
	else
	{
		const V3 ks = mk(p0.w, p1.x, p1.y);
		const float Ld = 0.212671f * kd.x + 0.715160f * kd.y + 0.072169f * kd.z;        // FColor::Luminance color.h:45-48
		const float Ls = 0.212671f * ks.x + 0.715160f * ks.y + 0.072169f * ks.z;
		const float Qd = Ld / (Ld + Ls);
		if (uplastic < Qd) { c.kind = CL_LAMBERT; c.c0 = kd / Qd; }
		else { c.kind = CL_MICROFACET; c.c0 = ks / (1 - Qd); c.fresnel = FR_DIELECTRIC; c.ax = c.ay = smax(0.001f, p1.z); }
	}
}
} // namespace jp
