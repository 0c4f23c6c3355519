/* include/jp_mipmap.h -- mip-mapped image textures (INTEGRATION.md "Mip maps"): the pyramid of an image, the ray cone a path carries, the footprint of the cone
 * in texels at a hit and the trilinear lookup, as the device kernels (k_mip_level, k_texel_m, k_mip_probe, k_guides*) and the host entry points
 * jp_build_mip_chain / jp_mip_cone_step / jp_mip_footprint / jp_texture_lookup_mip compute them.  This header is the one definition; tests/mipmap_ref.py restates
 * it in numpy float32 and agrees bit for bit.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off), and fp32
 * divide / sqrtf are the correctly rounded forms on the host and on the device.  Only + - * / sqrtf floorf, compares and integer operations on a float's bits: no
 * logarithm, no exp2f.  Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 *
 * Pyramid.  Level 0 is the image; level k + 1 has max(1, w_k >> 1) x max(1, h_k >> 1) texels, and its texel (i, j) is, per channel,
 * (a + b + c + d + 2) >> 2 over the source texels (2i, 2j), (2i + 1, 2j), (2i, 2j + 1), (2i + 1, 2j + 1), indices clamped to the source's size - 1 (an odd
 * size drops its last row / column except through that clamp; a 1-wide level averages each texel with itself).  Integers only.
 * L = 1 + floor(log2(max(w, h))) levels; level L - 1 is 1 x 1.  One dword per texel like level 0 (R | G << 8 | B << 16 | 0xff << 24).
 *
 * Cone.  Per path slot (width, spread).  gamma0 = 2 * |cam.up| / res_y is the pixel's spread (cam.up spans the image's height at distance 1).  At a hit at
 * distance t of a ray whose flags word is f:
 *   bounce 0       spread = gamma0,                                                     width = spread * t      (whatever the slot held)
 *   later bounces  spread = FLAG_SPEC(f) ? spread_prev : max(spread_prev, bounce_spread),  width = width_prev + spread * t
 * FLAG_SPEC on a QUEUED ray means "this ray left a specular closure": k_shade writes MK_FLAGS(nbounce, nspec, dim) into the next ray with
 * nspec = (bs.flags & BS_SPECULAR) != 0 of the BSDF sample that made the ray (integrator.cc:381), and k_raygen writes 0 for the camera ray.  A mirror or a
 * glass interface keeps the cone's spread; any other closure widens it to bounce_spread at least (a design constant, default 0.125 rad: roughly the half-angle
 * over which a glossy or diffuse lobe averages at the sample counts the guides exist for -- chosen, not measured).  The surface's curvature is ignored.
 *
 * Footprint.  A = |dpdu x dpdv|, the world area per unit of uv area at the hit, from the TRUE derivatives of every shape's GetUV (include/jp_normal_map.h's
 * tangents are the same directions, but only their directions matter there, so their lengths are restated here):
 *   triangle   |e1 x e2| / |det|, e1 = p1 - p0, e2 = p2 - p0, det = du1 dv2 - dv1 du2 of the colour uv set (jp_triangle_tangents_at's det); 0 where det is 0
 *              or not finite
 *   rectangle  |(p1 - p0) x (p3 - p0)|                        (u and v run 0 .. 1 along the two edges)
 *   sphere     2 pi^2 * r * sqrtf(d.x^2 + d.z^2), d = p - centre  (|dp/du| = 2 pi r cos(theta), |dp/dv| = pi r, orthogonal); 0 at the poles
 *   disk       2 pi * R * |p - centre|                           (|dp/du| = 2 pi |p - c|, |dp/dv| = R, orthogonal); 0 at the centre
 * rho = width * sqrtf(((w * scale_u) * (h * scale_v)) / A) * footprint_scale  texels.  ISOTROPIC: width is the cone's diameter, the MINOR axis of the ellipse
 * the cone projects on the surface.  No cosine term and no anisotropy clamp: a grazing view stays as sharp as a frontal one at the same distance, and the
 * aliasing along the ellipse's major axis is left to the pixel's samples (blur is the failure a path tracer cannot average away; aliasing it can).
 * rho = 0 (level 0) where rho is not finite, A is not finite or not > 0, or a triangle has no uv set.
 *
 * Level and fraction.  rho <= 1 (and rho = 0 above): exactly the lookup the texture has without mipmaps -- the record's nearest or bilinear filter, or the lookup
 * without records -- bit for bit what k_texel / k_texel_s write.  rho > 1: l = the unbiased exponent of rho, read from its bits (floor(log2(rho))), and
 * f = rho * 2^-l - 1, an exact multiplication by a power of two, so f lies in [0, 1).  l >= L - 1: bilinear on level L - 1 alone (the 1 x 1 level: its texel).
 * Else per channel bilinear on levels l and l + 1 (jp_tsamp_taps with the level's size and the record's wrap modes; the floats BEFORE quantisation),
 * r = r_l + f * (r_{l+1} - r_l), then one quantisation min((unsigned)(r + 0.5f), 255).  All eight texel loads are issued before the first use.
 * The coordinate is the record's (scale, offset, wrap); a texture without an active record takes the identity record (clamp).
 * A record whose filter is NEAREST (or a texture without a record, whose lookup is nearest) therefore has a small step at rho = 1: nearest on level 0 below,
 * bilinear between levels 0 and 1 with f = 0 just above -- at most the difference between a texel and the bilinear blend at that point.  Continuous for BILINEAR
 * records.
 */
#ifndef JP_MIPMAP_H
#define JP_MIPMAP_H
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "jetpbrt_amd.h"
#include "jp_counter_rng.h"      /* JP_HD */
#include "jp_tex_sampling.h"

#if defined(__HIPCC__)
#define JP_MIP_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_MIP_FN static inline
#endif

#define JP_MIP_MAX_LEVELS 15                 /* 16384 = 2^14 per side at the most */
#define JP_MIP_DEFAULT_BOUNCE_SPREAD 0.125f  /* radians; a design choice, not a measurement */
#define JP_MIP_2PI   6.2831855f
#define JP_MIP_2PI2  19.739209f              /* 2 pi^2 */

/* ---- pyramid ---- */
JP_MIP_FN int jp_mip_levels(int w, int h)
{
    int m = w > h ? w : h, n = 1;
    while (m > 1) { m >>= 1; n++; }
    return n;
}
JP_MIP_FN int jp_mip_half(int s) { return (s >> 1) > 1 ? (s >> 1) : 1; }

/* texel (i, j) of the level below a source level of sw x sh dwords */
JP_MIP_FN unsigned int jp_mip_down_texel(const unsigned int* src, int sw, int sh, int i, int j)
{
    const int i0 = 2 * i < sw - 1 ? 2 * i : sw - 1, i1 = 2 * i + 1 < sw - 1 ? 2 * i + 1 : sw - 1;
    const int j0 = 2 * j < sh - 1 ? 2 * j : sh - 1, j1 = 2 * j + 1 < sh - 1 ? 2 * j + 1 : sh - 1;
    const unsigned int a = src[(size_t)j0 * (size_t)sw + (size_t)i0], b = src[(size_t)j0 * (size_t)sw + (size_t)i1];
    const unsigned int c = src[(size_t)j1 * (size_t)sw + (size_t)i0], d = src[(size_t)j1 * (size_t)sw + (size_t)i1];
    unsigned int out = 0xff000000u;
    int k;
    for (k = 0; k < 3; k++)
        out |= ((((a >> (8 * k)) & 0xffu) + ((b >> (8 * k)) & 0xffu) + ((c >> (8 * k)) & 0xffu) + ((d >> (8 * k)) & 0xffu) + 2u) >> 2) << (8 * k);
    return out;
}

/* ---- cone ---- */
JP_MIP_FN void jp_mip_cone_hit(float gamma0, float bounce_spread, int flags, float t, float* width, float* spread)
{
    if ((flags & 0xff) == 0) { *spread = gamma0; *width = gamma0 * t; return; }
    if (!((flags >> 8) & 1)) *spread = *spread > bounce_spread ? *spread : bounce_spread;     /* max(spread_prev, bounce_spread); a NaN spread_prev gives bounce_spread */
    *width = *width + *spread * t;
}

/* ---- footprint ---- */
JP_MIP_FN float jp_mip_cross_len(const float a[3], const float b[3])
{
    const float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    return sqrtf((x * x + y * y) + z * z);
}
JP_MIP_FN float jp_mip_area_triangle(const float p0[3], const float p1[3], const float p2[3], const float uv6[6])
{
    const float du1 = uv6[2] - uv6[0], dv1 = uv6[3] - uv6[1], du2 = uv6[4] - uv6[0], dv2 = uv6[5] - uv6[1];
    const float det = du1 * dv2 - dv1 * du2;
    const float e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] }, e2[3] = { p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2] };
    if (det == 0.f || !(det - det == 0.f)) return 0.f;
    return jp_mip_cross_len(e1, e2) / (det < 0.f ? -det : det);
}
JP_MIP_FN float jp_mip_area_rectangle(const float p0[3], const float p1[3], const float p3[3])
{
    const float e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] }, e2[3] = { p3[0] - p0[0], p3[1] - p0[1], p3[2] - p0[2] };
    return jp_mip_cross_len(e1, e2);
}
JP_MIP_FN float jp_mip_area_sphere(const float d[3], float radius) { return (JP_MIP_2PI2 * radius) * sqrtf(d[0] * d[0] + d[2] * d[2]); }
JP_MIP_FN float jp_mip_area_disk(const float v0[3], float radius) { return (JP_MIP_2PI * radius) * sqrtf((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2]); }

/* rho in texels of level 0; w, h the image's size, su, sv the record's uv scale (1 without a record) */
JP_MIP_FN float jp_mip_rho(float width, float area, int w, int h, float su, float sv, float footprint_scale)
{
    if (!(area > 0.f) || !(area - area == 0.f)) return 0.f;
    const float rho = width * sqrtf((((float)w * su) * ((float)h * sv)) / area) * footprint_scale;
    return rho - rho == 0.f ? rho : 0.f;
}

/* ---- level and fraction ---- */
JP_MIP_FN unsigned int jp_mip_bits(float x) { unsigned int u; memcpy(&u, &x, 4); return u; }
JP_MIP_FN float jp_mip_from_bits(unsigned int u) { float x; memcpy(&x, &u, 4); return x; }
/* rho > 1, finite: its unbiased exponent (0 .. 127) */
JP_MIP_FN int jp_mip_level_of(float rho) { return (int)((jp_mip_bits(rho) >> 23) & 0xffu) - 127; }
/* rho > 1, l = jp_mip_level_of(rho) < 127: rho * 2^-l - 1 in [0, 1) */
JP_MIP_FN float jp_mip_fraction(float rho, int l) { return rho * jp_mip_from_bits((unsigned int)(127 - l) << 23) - 1.f; }

/* the identity record a texture without an active one is addressed through above level 0 */
JP_MIP_FN JpTexSampler jp_mip_identity_sampler(void)
{
    JpTexSampler s;
    s.wrap_u = JP_WRAP_CLAMP; s.wrap_v = JP_WRAP_CLAMP; s.filter = JP_FILTER_DEFAULT; s.scale_u = 1.f; s.scale_v = 1.f; s.offset_u = 0.f; s.offset_v = 0.f;
    return s;
}

/* one level of the pyramid as the lookup sees it: size and the first texel relative to `texels` (the pool holds at most 2^31 texels) */
typedef struct JpMipLevel { int32_t w, h, first, pad; } JpMipLevel;     /* 16 bytes: the device's level table is an array of these */

JP_MIP_FN float jp_mip_bilerp(float a, float b, float c, float d, float fx, float fy)
{
    const float r0 = a + fx * (b - a), r1 = c + fx * (d - c);
    return r0 + fy * (r1 - r0);
}

/* rho > 1 on a pyramid of n_levels levels: R | G << 8 | B << 16.  s: the record (never null: jp_mip_identity_sampler without one) */
JP_MIP_FN unsigned int jp_mip_lookup_above(const JpTexSampler* s, const unsigned int* texels, const JpMipLevel* lev, int n_levels, float uu, float vv, float rho)
{
    const float u = jp_tsamp_coord(uu, s->scale_u, s->offset_u, s->wrap_u);
    const float vf = 1.f - jp_tsamp_coord(vv, s->scale_v, s->offset_v, s->wrap_v);
    const int l = jp_mip_level_of(rho);
    unsigned int out = 0u;
    int k;
    if (l >= n_levels - 1)
    {
        const JpMipLevel a = lev[n_levels - 1];
        const JpTsampTaps t = jp_tsamp_taps(s, a.w, a.h, u, vf);
        const unsigned int* p = texels + (size_t)a.first;
        const unsigned int t00 = p[t.k00], t10 = p[t.k10], t01 = p[t.k01], t11 = p[t.k11];
        for (k = 0; k < 3; k++)
            out |= jp_tsamp_byte((float)((t00 >> (8 * k)) & 0xffu), (float)((t10 >> (8 * k)) & 0xffu), (float)((t01 >> (8 * k)) & 0xffu), (float)((t11 >> (8 * k)) & 0xffu), t.fx, t.fy) << (8 * k);
        return out;
    }
    {
        const float f = jp_mip_fraction(rho, l);
        const JpMipLevel a = lev[l], b = lev[l + 1];
        const JpTsampTaps ta = jp_tsamp_taps(s, a.w, a.h, u, vf), tb = jp_tsamp_taps(s, b.w, b.h, u, vf);
        const unsigned int* pa = texels + (size_t)a.first;
        const unsigned int* pb = texels + (size_t)b.first;
        const unsigned int a00 = pa[ta.k00], a10 = pa[ta.k10], a01 = pa[ta.k01], a11 = pa[ta.k11];     /* all eight before the first use */
        const unsigned int b00 = pb[tb.k00], b10 = pb[tb.k10], b01 = pb[tb.k01], b11 = pb[tb.k11];
        for (k = 0; k < 3; k++)
        {
            const float ra = jp_mip_bilerp((float)((a00 >> (8 * k)) & 0xffu), (float)((a10 >> (8 * k)) & 0xffu), (float)((a01 >> (8 * k)) & 0xffu), (float)((a11 >> (8 * k)) & 0xffu), ta.fx, ta.fy);
            const float rb = jp_mip_bilerp((float)((b00 >> (8 * k)) & 0xffu), (float)((b10 >> (8 * k)) & 0xffu), (float)((b01 >> (8 * k)) & 0xffu), (float)((b11 >> (8 * k)) & 0xffu), tb.fx, tb.fy);
            const float q = (ra + f * (rb - ra)) + 0.5f;
            const unsigned int v = q > 0.f ? (unsigned int)q : 0u;
            out |= (v < 255u ? v : 255u) << (8 * k);
        }
    }
    return out;
}

/* host side only: what jp_set_texture_mipmaps accepts: 0, or the first rule broken -- 1 a mode unknown (texture *bad), 2 footprint_scale, 3 bounce_spread */
static inline int jp_mipmaps_check(const JpTextureMipmaps* m, int* bad, int* n_on)
{
    int i;
    *bad = -1; *n_on = 0;
    if (m->mode) for (i = 0; i < m->n_textures; i++)
    {
        if (m->mode[i] != JP_MIP_OFF && m->mode[i] != JP_MIP_TRILINEAR) { *bad = i; return 1; }
        if (m->mode[i] == JP_MIP_TRILINEAR) (*n_on)++;
    }
    if (!(m->footprint_scale - m->footprint_scale == 0.f) || !(m->footprint_scale >= 0.f)) return 2;
    if (!(m->bounce_spread - m->bounce_spread == 0.f) || !(m->bounce_spread >= 0.f)) return 3;
    return 0;
}
static inline const char* jp_mipmaps_rule(int rule)
{
    switch (rule)
    {
    case 1: return "unknown mode (JP_MIP_OFF, JP_MIP_TRILINEAR)";
    case 2: return "footprint_scale must be finite and >= 0 (0: the default, 1)";
    case 3: return "bounce_spread must be finite and >= 0 (0: the default, 0.125 rad)";
    default: return "";
    }
}
#endif
