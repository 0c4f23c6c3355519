/* include/jp_tex_sampling.h -- texture sampling records (INTEGRATION.md "Texture sampling"): a wrap mode per axis, a uv scale and offset and a filter for an
 * image texture or a normal map, as the device kernels (k_texel_s, k_normal_map_s, k_surface, k_guides*, k_shading_normal_mapped) and the host entry points
 * jp_texture_lookup / jp_perturb_normals_sampled compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off).  Only
 * + - *, floorf and compares; no float-to-int cast sees a value outside the int range or a NaN (tools/tex_sampling_host_check.cpp runs the edge set under
 * the address and undefined-behaviour sanitizers).  Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 *
 * Coordinate, per axis: t = c * scale + offset.  A t that is not finite gives 0; else
 *   CLAMP   t < 0 ? 0 : (t > 1 ? 1 : t)
 *   REPEAT  t - floorf(t)                       (exactly 1 for a tiny negative t: the index rules below define that case)
 *   MIRROR  k = floorf(t), f = t - k;  1 - f when k - 2 * floorf(k * 0.5f) == 1, else f
 * then v is flipped, v' = 1 - v (row 0 is the top row).
 * NEAREST:  i = (int)(u * w), j = (int)(v' * h), each clamped to size - 1; colour (1.0f / 255.0f) * byte.
 * BILINEAR: x = u * w - 0.5f, x0 = floorf(x), fx = x - x0, columns x0 and x0 + 1 (y likewise with v'); an index out of range is taken modulo the size on a REPEAT
 *   axis and clamped on a CLAMP or MIRROR axis (across a mirrored edge the neighbour is the same texel); per channel r0 = a + fx * (b - a), r1 = c + fx * (d - c),
 *   r = r0 + fy * (r1 - r0).  A colour texture returns the byte min((unsigned)(r + 0.5f), 255) -- the filtered colour is quantised to 8 bits, at most half a step of
 *   the source's own quantisation -- in the 24-bit side word of the nearest lookup; a normal map decodes the four texels (jp_nmap_decode) and interpolates the floats.
 * DEFAULT is NEAREST for a colour texture and BILINEAR for a normal map.
 * The identity record -- both wraps CLAMP, the filter DEFAULT or the kind's own default, scale (1, 1), offset (0, 0) -- and no record at all select the lookup
 * without records (FImageTexture::Sample: clamp, flip, nearest; jp_nmap_lookup for a normal map), which the rules above reproduce for every finite coordinate;
 * for a coordinate that is not finite that lookup keeps its own answer (+inf clamps to 1, a NaN selects texel 0 on its axis).
 */
#ifndef JP_TEX_SAMPLING_H
#define JP_TEX_SAMPLING_H
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "jetpbrt_amd.h"         /* JpTexSampler, JP_WRAP_*, JP_FILTER_* */
#include "jp_counter_rng.h"      /* JP_HD */
#include "jp_normal_map.h"      /* jp_nmap_decode, jp_nmap_lookup, jp_nmap_apply */

#if defined(__HIPCC__)
#define JP_TSAMP_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_TSAMP_FN static inline
#endif

enum { JP_TSAMP_COLOR = 0, JP_TSAMP_NORMAL = 1 };      /* the kind of image a record addresses */

/* one axis: transform, then wrap */
JP_TSAMP_FN float jp_tsamp_coord(float c, float scale, float offset, int wrap)
{
    const float t = c * scale + offset;
    if (!(t - t == 0.f)) return 0.f;
    if (wrap == JP_WRAP_REPEAT) return t - floorf(t);
    if (wrap == JP_WRAP_MIRROR)
    {
        const float k = floorf(t), f = t - k;
        return k - 2.f * floorf(k * 0.5f) == 1.f ? 1.f - f : f;
    }
    return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
}

/* a bilinear tap's index (-1 .. size) on its axis */
JP_TSAMP_FN int jp_tsamp_index(int i, int size, int wrap)
{
    if (wrap == JP_WRAP_REPEAT) return i < 0 ? i + size : (i >= size ? i - size : i);
    return i < 0 ? 0 : (i > size - 1 ? size - 1 : i);
}

/* the lookup without records of a colour texture (FImageTexture::Sample): the texel's index */
JP_TSAMP_FN size_t jp_tsamp_nearest_clamp(int w, int h, float uu, float vv)
{
    const float u = uu < 0.f ? 0.f : (uu > 1.f ? 1.f : uu);
    const float v = 1.f - (vv < 0.f ? 0.f : (vv > 1.f ? 1.f : vv));
    const float fi = u * (float)w, fj = v * (float)h;
    int i = fi >= 0.f ? (int)fi : 0, j = fj >= 0.f ? (int)fj : 0;
    if (i >= w) i = w - 1;
    if (j >= h) j = h - 1;
    return (size_t)j * (size_t)w + (size_t)i;
}

/* the four taps of a bilinear lookup and its two weights */
typedef struct JpTsampTaps { size_t k00, k10, k01, k11; float fx, fy; } JpTsampTaps;
JP_TSAMP_FN JpTsampTaps jp_tsamp_taps(const JpTexSampler* s, int w, int h, float u, float vf)
{
    JpTsampTaps t;
    const float x = u * (float)w - 0.5f, y = vf * (float)h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const int i0 = jp_tsamp_index((int)x0, w, s->wrap_u), i1 = jp_tsamp_index((int)x0 + 1, w, s->wrap_u);
    const int j0 = jp_tsamp_index((int)y0, h, s->wrap_v), j1 = jp_tsamp_index((int)y0 + 1, h, s->wrap_v);
    t.fx = x - x0; t.fy = y - y0;
    t.k00 = (size_t)j0 * (size_t)w + (size_t)i0; t.k10 = (size_t)j0 * (size_t)w + (size_t)i1;
    t.k01 = (size_t)j1 * (size_t)w + (size_t)i0; t.k11 = (size_t)j1 * (size_t)w + (size_t)i1;
    return t;
}

JP_TSAMP_FN unsigned int jp_tsamp_byte(float a, float b, float c, float d, float fx, float fy)
{
    const float r0 = a + fx * (b - a), r1 = c + fx * (d - c);
    const float q = (r0 + fy * (r1 - r0)) + 0.5f;
    const unsigned int v = q > 0.f ? (unsigned int)q : 0u;
    return v < 255u ? v : 255u;
}

/* a colour texture under an ACTIVE record: R | G << 8 | B << 16 of the answer; texels: one dword per texel, R | G << 8 | B << 16, row-major, top row first */
JP_TSAMP_FN unsigned int jp_tex_lookup_sampled(const JpTexSampler* s, const unsigned int* texels, int w, int h, float uu, float vv)
{
    const float u = jp_tsamp_coord(uu, s->scale_u, s->offset_u, s->wrap_u);
    const float vf = 1.f - jp_tsamp_coord(vv, s->scale_v, s->offset_v, s->wrap_v);
    if (s->filter != JP_FILTER_BILINEAR)
    {
        int i = (int)(u * (float)w), j = (int)(vf * (float)h);
        if (i > w - 1) i = w - 1;
        if (j > h - 1) j = h - 1;
        return texels[(size_t)j * (size_t)w + (size_t)i] & 0xffffffu;
    }
    const JpTsampTaps t = jp_tsamp_taps(s, w, h, u, vf);
    const unsigned int t00 = texels[t.k00], t10 = texels[t.k10], t01 = texels[t.k01], t11 = texels[t.k11];    /* all four before the first use */
    unsigned int out = 0u;
    int k;
    for (k = 0; k < 3; k++)
        out |= jp_tsamp_byte((float)((t00 >> (8 * k)) & 0xffu), (float)((t10 >> (8 * k)) & 0xffu), (float)((t01 >> (8 * k)) & 0xffu), (float)((t11 >> (8 * k)) & 0xffu), t.fx, t.fy) << (8 * k);
    return out;
}

/* a normal map under an ACTIVE record (its filter is bilinear): the tangent-space vector before the strength, as jp_nmap_lookup delivers it */
JP_TSAMP_FN void jp_nmap_lookup_sampled(const JpTexSampler* s, const unsigned int* texels, int w, int h, float uu, float vv, float m[3])
{
    const float u = jp_tsamp_coord(uu, s->scale_u, s->offset_u, s->wrap_u);
    const float vf = 1.f - jp_tsamp_coord(vv, s->scale_v, s->offset_v, s->wrap_v);
    const JpTsampTaps t = jp_tsamp_taps(s, w, h, u, vf);
    const unsigned int t00 = texels[t.k00], t10 = texels[t.k10], t01 = texels[t.k01], t11 = texels[t.k11];
    int k;
    for (k = 0; k < 3; k++)
    {
        const float a = jp_nmap_decode((t00 >> (8 * k)) & 0xffu), b = jp_nmap_decode((t10 >> (8 * k)) & 0xffu);
        const float c = jp_nmap_decode((t01 >> (8 * k)) & 0xffu), d = jp_nmap_decode((t11 >> (8 * k)) & 0xffu);
        const float r0 = a + t.fx * (b - a), r1 = c + t.fx * (d - c);
        m[k] = r0 + t.fy * (r1 - r0);
    }
}

/* lookup + apply under a record; s null: jp_perturb_normal */
JP_TSAMP_FN int jp_perturb_normal_sampled(const JpTexSampler* s, const float nb[3], const float ng[3], const float dpdu[3], const float dpdv[3], float u, float v,
                                          const unsigned int* texels, int w, int h, float strength, float ns[3])
{
    float m[3];
    if (s) jp_nmap_lookup_sampled(s, texels, w, h, u, v, m);
    else jp_nmap_lookup(texels, w, h, u, v, m);
    return jp_nmap_apply(nb, ng, dpdu, dpdv, m, strength, ns);
}

/* is the record the identity of its kind: the lookup without records */
JP_TSAMP_FN int jp_tsamp_identity(const JpTexSampler* s, int kind)
{
    const int own = kind == JP_TSAMP_NORMAL ? JP_FILTER_BILINEAR : JP_FILTER_NEAREST;
    return s->wrap_u == JP_WRAP_CLAMP && s->wrap_v == JP_WRAP_CLAMP && (s->filter == JP_FILTER_DEFAULT || s->filter == own)
        && s->scale_u == 1.f && s->scale_v == 1.f && s->offset_u == 0.f && s->offset_v == 0.f;
}

/* host side only: what jp_set_texture_sampling accepts for one record: 0, or the index of the first rule broken -- 1 wrap unknown, 2 filter unknown,
 * 3 a scale not finite or not > 0, 4 an offset not finite, 5 MIRROR on a normal map, 6 NEAREST on a normal map */
static inline int jp_tex_sampler_check(const JpTexSampler* s, int kind)
{
    if (s->wrap_u < JP_WRAP_CLAMP || s->wrap_u > JP_WRAP_MIRROR || s->wrap_v < JP_WRAP_CLAMP || s->wrap_v > JP_WRAP_MIRROR) return 1;
    if (s->filter < JP_FILTER_DEFAULT || s->filter > JP_FILTER_BILINEAR) return 2;
    if (!(s->scale_u - s->scale_u == 0.f) || !(s->scale_u > 0.f) || !(s->scale_v - s->scale_v == 0.f) || !(s->scale_v > 0.f)) return 3;
    if (!(s->offset_u - s->offset_u == 0.f) || !(s->offset_v - s->offset_v == 0.f)) return 4;
    if (kind == JP_TSAMP_NORMAL && (s->wrap_u == JP_WRAP_MIRROR || s->wrap_v == JP_WRAP_MIRROR)) return 5;
    if (kind == JP_TSAMP_NORMAL && s->filter == JP_FILTER_NEAREST) return 6;
    return 0;
}
static inline const char* jp_tex_sampler_rule(int rule)
{
    switch (rule)
    {
    case 1: return "unknown wrap mode (JP_WRAP_CLAMP, JP_WRAP_REPEAT, JP_WRAP_MIRROR)";
    case 2: return "unknown filter (JP_FILTER_DEFAULT, JP_FILTER_NEAREST, JP_FILTER_BILINEAR)";
    case 3: return "scale must be finite and > 0";
    case 4: return "offset not finite";
    case 5: return "JP_WRAP_MIRROR on a normal map would need tangent sign changes (CLAMP or REPEAT)";
    case 6: return "a normal map is filtered bilinearly (JP_FILTER_DEFAULT or JP_FILTER_BILINEAR)";
    default: return "";
    }
}
#endif
