/* include/jp_procedural.h -- procedural textures (INTEGRATION.md "Procedural textures"): gradient noise, fBm, turbulence, marble and the box-filtered 3D checker,
 * band-limited by the footprint of the path's ray cone, as the device kernels (k_texel_p, k_proc_probe, k_guides*) and the host entry point jp_procedural_lookup
 * compute them.  This header is the one definition; tests/procedural_ref.py restates it in numpy float32 and agrees bit for bit.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off), and fp32
 * divide / sqrtf are the correctly rounded forms on the host and on the device.  Only + - * / sqrtf floorf, compares and integer operations: no sine, no
 * logarithm, no exp2f -- with ONE exception, the plain checker below its footprint threshold (see CHECKER_AA), which is the lookup the texture has without a
 * record.  Every float-to-int conversion is guarded: no input bits (NaN, infinity, |x| >= 2^24) reach an undefined conversion.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 *
 * Point.  x = the hit point p (JP_PROC_SPACE_WORLD) or (u, v, 0) (JP_PROC_SPACE_UV); q = M x + t, row by row: q_r = ((m[4r] * x0 + m[4r+1] * x1) + m[4r+2] * x2) + m[4r+3].
 * "q is in range": every q_r is finite and |q_r| < 2^24.
 *
 * Noise n(q).  Perlin's improved noise on the integer lattice.  q out of range: 0.  Else per axis f = floorf(q), i = (int)f, x = q - f in [0, 1); the hash of
 * the corner (i + dx, j + dy, k + dz) is jp_rng_key(JP_PROC_SEED, i + dx, j + dy, k + dz) of include/jp_counter_rng.h (integers wrap as uint32) -- a chain of
 * jp_mix32, so the two x keys, four xy keys and eight corner keys of a cell share their prefixes; no table, no memory traffic.  The gradient is Perlin's grad on the
 * hash's low 4 bits: u = h < 8 ? x : y; v = h < 4 ? y : (h == 12 || h == 14 ? x : z); g = ((h & 1) ? -u : u) + ((h & 2) ? -v : v), at the corner's own offset
 * (x - dx, y - dy, z - dz).  Fade (Horner): w(t) = ((t * t) * t) * (t * (t * 6 - 15) + 10).  Blend x, then y, then z, each as a + w * (b - a).  The result is
 * clamped to [-1, 1] (the unclamped blend of these twelve gradients can exceed 1 by a few per cent off the cell's centre).  At a lattice point x = y = z = 0 and
 * n = grad(h, 0, 0, 0) = 0 exactly.
 *
 * Footprint.  fw = width * s: width the cone's width at the hit (include/jp_mipmap.h; the number jp_mip_rho takes), s = sqrtf of the largest squared column
 * norm of M's linear part, computed once by jp_proc_resolve.  antialias off: s = 0.  fw that is not > 0 (a NaN among them) counts as 0.
 *
 * Octave weight.  Octave i: frequency 2^i, amplitude gain^i (amp_0 = 1, amp_{i+1} = amp_i * gain), k_i = fw * 2^i (k_0 = fw, k_{i+1} = k_i * 2: exact).
 * a_i = 1 for k_i <= 0.25, 0 for k_i >= 0.5, else (0.5 - k_i) * 4.  The a_i never increase, and the loop stops at the first a_i = 0.
 *   sum_fbm  = sum over i of (a_i * amp_i) * n(f_i q), f_0 = 1, f_{i+1} = f_i * 2, each coordinate of q scaled by f_i; accumulated in octave order from 0
 *   sum_turb = sum over i of (a_i * amp_i) * |n(f_i q)| + ((1 - a_i) * amp_i) * 0.2f, the octaves from the first a_i = 0 on adding amp_i * 0.2f each
 * norm = 1 / (sum of amp_i over the record's octaves), fp32 in octave order (jp_proc_resolve).
 *
 * Kinds.  clamp01(x) = !(x > 0) ? 0 : (x > 1 ? 1 : x)  (NaN: 0).
 *   NOISE       t = clamp01(0.5 + 0.5 * (a_0 * n(q)))
 *   FBM         t = clamp01(0.5 + 0.5 * (norm * sum_fbm))
 *   TURBULENCE  t = clamp01(norm * sum_turb)
 *   MARBLE      s = q_y + variation * sum_fbm; y = clamp01(2 * |s - floorf(s + 0.5f)|); t = (y * y) * (3 - 2 * y)
 *   colour, per channel: r = c_even + t * (c_odd - c_even); byte = q > 0 ? (q < 256 ? (unsigned)q : 255) : 0 with q = 255 * r + 0.5f; word = JP_TEX_IMAGE_TAG | R | G << 8 | B << 16
 *   CHECKER_AA  q out of range: t = 0.5.  Else, with y_r = q_r * JP_PROC_10_OVER_PI (the checker's square wave sign(sin(10 x)) has period 2 in y) and
 *               fy = fw * JP_PROC_10_OVER_PI:
 *                 fy <= JP_PROC_CHECKER_MIN (1/32: 1/64 of the period): the PLAIN checker's own word, JP_TEX_COLOR_TAG | (2 * texture + (sx * sy * sz < 0 ? 0 : 1)),
 *                   sx = sin(10 * q_x) etc. (the host's sincosf; the device's sincos_f) -- with the identity map exactly what tex_sample writes; t = 1 (odd) or 0
 *                 fy >= JP_PROC_CHECKER_MAX (4096) or not finite: t = 0.5 exactly
 *                 else per axis m = (T(y + fy / 2) - T(y - fy / 2)) / fy, T(y) the integral of the square wave: r = y - 2 * floorf(y * 0.5f), T = r < 1 ? r : 2 - r;
 *                   m clamped to [-1, 1]; t = (1 - (m_x * m_y) * m_z) * 0.5, the odd fraction
 */
#ifndef JP_PROCEDURAL_H
#define JP_PROCEDURAL_H
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "jetpbrt_amd.h"
#include "jp_counter_rng.h"      /* JP_HD, jp_mix32 */

#if defined(__HIPCC__)
#define JP_PROC_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_PROC_FN static inline
#endif

#define JP_PROC_SEED         0x50524f43u     /* "PROC" */
#define JP_PROC_MAX_OCTAVES  12
#define JP_PROC_DEFAULT_OCTAVES 6
#define JP_PROC_LIMIT        16777216.f      /* 2^24 */
#define JP_PROC_10_OVER_PI   3.1830988f      /* 10 / pi */
#define JP_PROC_CHECKER_MIN  0.03125f
#define JP_PROC_CHECKER_MAX  4096.f
#define JP_PROC_TAG_IMAGE    0x80000000u     /* JP_TEX_IMAGE_TAG / JP_TEX_COLOR_TAG of the side word (csrc/jp_common.h) */
#define JP_PROC_TAG_COLOR    0x40000000u

/* the record as the lookup reads it: defaults resolved, norm and s computed (jp_proc_resolve); 80 bytes, the device's table is an array of these */
typedef struct JpProcDev { int32_t kind, space, octaves, pad; float m[12]; float gain, variation, norm, s; } JpProcDev;

JP_PROC_FN int jp_proc_in_range(float x) { return x - x == 0.f && x > -JP_PROC_LIMIT && x < JP_PROC_LIMIT; }
JP_PROC_FN float jp_proc_clamp01(float x) { return !(x > 0.f) ? 0.f : (x > 1.f ? 1.f : x); }

JP_PROC_FN float jp_proc_grad(uint32_t hash, float x, float y, float z)
{
    const uint32_t h = hash & 15u;
    const float u = h < 8u ? x : y;
    const float v = h < 4u ? y : ((h == 12u || h == 14u) ? x : z);
    return ((h & 1u) ? -u : u) + ((h & 2u) ? -v : v);
}
JP_PROC_FN float jp_proc_fade(float t) { return ((t * t) * t) * (t * (t * 6.f - 15.f) + 10.f); }

JP_PROC_FN float jp_proc_noise(float qx, float qy, float qz)
{
    if (!jp_proc_in_range(qx) || !jp_proc_in_range(qy) || !jp_proc_in_range(qz)) return 0.f;
    {
        const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
        const uint32_t ix = (uint32_t)(int32_t)fx, iy = (uint32_t)(int32_t)fy, iz = (uint32_t)(int32_t)fz;     /* |f| <= 2^24: in range */
        const float x = qx - fx, y = qy - fy, z = qz - fz;
        const float x1 = x - 1.f, y1 = y - 1.f, z1 = z - 1.f;
        /* jp_rng_key(JP_PROC_SEED, i, j, k) with the shared prefixes hoisted; the eight corner keys depend on nothing but these and issue together */
        const uint32_t k0 = jp_mix32(JP_PROC_SEED ^ 0x9E3779B9U);
        const uint32_t ka = jp_mix32(k0 + ix), kb = jp_mix32(k0 + (ix + 1u));
        const uint32_t kaa = jp_mix32(ka + iy), kba = jp_mix32(kb + iy), kab = jp_mix32(ka + (iy + 1u)), kbb = jp_mix32(kb + (iy + 1u));
        const uint32_t h000 = jp_mix32(kaa + iz), h100 = jp_mix32(kba + iz), h010 = jp_mix32(kab + iz), h110 = jp_mix32(kbb + iz);
        const uint32_t h001 = jp_mix32(kaa + (iz + 1u)), h101 = jp_mix32(kba + (iz + 1u)), h011 = jp_mix32(kab + (iz + 1u)), h111 = jp_mix32(kbb + (iz + 1u));
        const float g000 = jp_proc_grad(h000, x, y, z), g100 = jp_proc_grad(h100, x1, y, z), g010 = jp_proc_grad(h010, x, y1, z), g110 = jp_proc_grad(h110, x1, y1, z);
        const float g001 = jp_proc_grad(h001, x, y, z1), g101 = jp_proc_grad(h101, x1, y, z1), g011 = jp_proc_grad(h011, x, y1, z1), g111 = jp_proc_grad(h111, x1, y1, z1);
        const float u = jp_proc_fade(x), v = jp_proc_fade(y), w = jp_proc_fade(z);
        const float a = g000 + u * (g100 - g000), b = g010 + u * (g110 - g010), c = g001 + u * (g101 - g001), d = g011 + u * (g111 - g011);
        const float e = a + v * (b - a), f = c + v * (d - c);
        const float n = e + w * (f - e);
        return n < -1.f ? -1.f : (n > 1.f ? 1.f : n);
    }
}

JP_PROC_FN float jp_proc_weight(float k) { return k <= 0.25f ? 1.f : (k >= 0.5f ? 0.f : (0.5f - k) * 4.f); }

/* sum_fbm (turb 0) or sum_turb (turb 1) */
JP_PROC_FN float jp_proc_octaves(const float q[3], float fw, int octaves, float gain, int turb)
{
    float sum = 0.f, amp = 1.f, f = 1.f, k = fw;
    int i = 0;
    for (; i < octaves; i++)
    {
        const float a = jp_proc_weight(k);
        float n;
        if (a == 0.f) break;
        n = jp_proc_noise(f * q[0], f * q[1], f * q[2]);
        if (turb) sum = sum + ((a * amp) * (n < 0.f ? -n : n) + ((1.f - a) * amp) * 0.2f);
        else sum = sum + (a * amp) * n;
        amp = amp * gain; f = f * 2.f; k = k * 2.f;
    }
    if (turb) for (; i < octaves; i++) { sum = sum + amp * 0.2f; amp = amp * gain; }
    return sum;
}

JP_PROC_FN float jp_proc_tri_integral(float y)
{
    const float r = y - 2.f * floorf(y * 0.5f);
    return r < 1.f ? r : 2.f - r;
}
JP_PROC_FN float jp_proc_square_mean(float y, float fy)
{
    const float h = fy * 0.5f;
    const float m = (jp_proc_tri_integral(y + h) - jp_proc_tri_integral(y - h)) / fy;
    return m < -1.f ? -1.f : (m > 1.f ? 1.f : m);
}

JP_PROC_FN unsigned int jp_proc_byte(float r)
{
    const float q = 255.f * r + 0.5f;
    return q > 0.f ? (q < 256.f ? (unsigned int)q : 255u) : 0u;
}
JP_PROC_FN unsigned int jp_proc_word(const float c_even[3], const float c_odd[3], float t)
{
    unsigned int out = JP_PROC_TAG_IMAGE;
    int k;
    for (k = 0; k < 3; k++) out |= jp_proc_byte(c_even[k] + t * (c_odd[k] - c_even[k])) << (8 * k);
    return out;
}

JP_PROC_FN void jp_proc_point(const JpProcDev* r, const float p[3], float u, float v, float q[3])
{
    const float x0 = r->space == JP_PROC_SPACE_UV ? u : p[0], x1 = r->space == JP_PROC_SPACE_UV ? v : p[1], x2 = r->space == JP_PROC_SPACE_UV ? 0.f : p[2];
    int k;
    for (k = 0; k < 3; k++) q[k] = ((r->m[4 * k] * x0 + r->m[4 * k + 1] * x1) + r->m[4 * k + 2] * x2) + r->m[4 * k + 3];
}

/* the side word of texture `texture` (its record r, kind not NONE) at the hit; *t_out: the blend parameter */
JP_PROC_FN unsigned int jp_proc_lookup(const JpProcDev* r, const float c_even[3], const float c_odd[3], int texture, const float p[3], float u, float v, float width, float* t_out)
{
    float q[3], fw = width * r->s, t;
    jp_proc_point(r, p, u, v, q);
    if (!(fw > 0.f)) fw = 0.f;
    if (r->kind == JP_PROC_CHECKER_AA)
    {
        const float fy = fw * JP_PROC_10_OVER_PI;
        if (!jp_proc_in_range(q[0]) || !jp_proc_in_range(q[1]) || !jp_proc_in_range(q[2])) t = 0.5f;
        else if (fy <= JP_PROC_CHECKER_MIN)
        {
            float sx, sy, sz, c;
#if defined(__HIP_DEVICE_COMPILE__)
            JP_PROC_SINCOSF_DEVICE(10 * q[0], &sx, &c); JP_PROC_SINCOSF_DEVICE(10 * q[1], &sy, &c); JP_PROC_SINCOSF_DEVICE(10 * q[2], &sz, &c);
#else
            sincosf(10 * q[0], &sx, &c); sincosf(10 * q[1], &sy, &c); sincosf(10 * q[2], &sz, &c);
#endif
            {
                const unsigned int even = !(sx * sy * sz < 0.0f) ? 1u : 0u;
                *t_out = even ? 0.f : 1.f;
                return JP_PROC_TAG_COLOR | (2u * (unsigned int)texture + even);
            }
        }
        else if (!(fy < JP_PROC_CHECKER_MAX)) t = 0.5f;
        else
        {
            const float mx = jp_proc_square_mean(q[0] * JP_PROC_10_OVER_PI, fy), my = jp_proc_square_mean(q[1] * JP_PROC_10_OVER_PI, fy), mz = jp_proc_square_mean(q[2] * JP_PROC_10_OVER_PI, fy);
            t = (1.f - (mx * my) * mz) * 0.5f;
        }
    }
    else if (r->kind == JP_PROC_NOISE) t = jp_proc_clamp01(0.5f + 0.5f * (jp_proc_weight(fw) * jp_proc_noise(q[0], q[1], q[2])));
    else if (r->kind == JP_PROC_FBM) t = jp_proc_clamp01(0.5f + 0.5f * (r->norm * jp_proc_octaves(q, fw, r->octaves, r->gain, 0)));
    else if (r->kind == JP_PROC_TURBULENCE) t = jp_proc_clamp01(r->norm * jp_proc_octaves(q, fw, r->octaves, r->gain, 1));
    else
    {
        const float s = q[1] + r->variation * jp_proc_octaves(q, fw, r->octaves, r->gain, 0);
        const float d = s - floorf(s + 0.5f);
        const float y = jp_proc_clamp01(2.f * (d < 0.f ? -d : d));
        t = (y * y) * (3.f - 2.f * y);
    }
    *t_out = t;
    return jp_proc_word(c_even, c_odd, t);
}

/* ---- host side only ---- */
/* what a record must satisfy by itself: 0, or the first rule broken */
static inline int jp_procedural_check(const JpProcedural* r)
{
    int k;
    if (r->kind < JP_PROC_NONE || r->kind > JP_PROC_CHECKER_AA) return 1;
    if (r->kind == JP_PROC_NONE) return 0;
    if (r->space != JP_PROC_SPACE_WORLD && r->space != JP_PROC_SPACE_UV) return 2;
    for (k = 0; k < 12; k++) if (!(r->m[k] - r->m[k] == 0.f)) return 3;
    {
        const float* m = r->m;
        const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
        if (det == 0.f || !(det - det == 0.f)) return 4;
    }
    if (r->octaves < 0 || r->octaves > JP_PROC_MAX_OCTAVES) return 5;
    if (!(r->gain - r->gain == 0.f) || r->gain < 0.f || r->gain > 1.f) return 6;
    if (!(r->variation - r->variation == 0.f)) return 7;
    if (r->antialias < -1 || r->antialias > 1) return 8;
    return 0;
}
static inline const char* jp_procedural_rule(int rule)
{
    switch (rule)
    {
    case 1: return "unknown kind (JP_PROC_NONE .. JP_PROC_CHECKER_AA)";
    case 2: return "unknown space (JP_PROC_SPACE_WORLD, JP_PROC_SPACE_UV)";
    case 3: return "m must be finite";
    case 4: return "the linear part of m is singular";
    case 5: return "octaves must be 0 (the default, 6) or 1 .. 12";
    case 6: return "gain must be 0 (the default, 0.5) or in (0, 1]";
    case 7: return "variation must be finite (0: the default, 1)";
    case 8: return "antialias must be 0 (the default: on), 1 or -1";
    case 9: return "a procedural record on a texture that is not JP_TEXTURE_CHECKER";
    case 10: return "the texture's two colours must lie in [0, 1] (the result is an RGB8 side word)";
    case 11: return "JP_PROC_SPACE_UV on a scene whose triangles have no tri_uv";
    default: return "";
    }
}
/* the record the lookup reads, from one that passed jp_procedural_check (kind not NONE) */
static inline JpProcDev jp_proc_resolve(const JpProcedural* r)
{
    JpProcDev d;
    int k;
    float acc = 0.f, amp = 1.f, best = 0.f;
    d.kind = r->kind; d.space = r->space; d.pad = 0;
    d.octaves = r->kind == JP_PROC_NOISE ? 1 : (r->octaves == 0 ? JP_PROC_DEFAULT_OCTAVES : r->octaves);
    for (k = 0; k < 12; k++) d.m[k] = r->m[k];
    d.gain = r->gain == 0.f ? 0.5f : r->gain;
    d.variation = r->variation == 0.f ? 1.f : r->variation;
    for (k = 0; k < d.octaves; k++) { acc = acc + amp; amp = amp * d.gain; }
    d.norm = 1.f / acc;
    for (k = 0; k < 3; k++)
    {
        const float n2 = (r->m[k] * r->m[k] + r->m[4 + k] * r->m[4 + k]) + r->m[8 + k] * r->m[8 + k];
        if (n2 > best) best = n2;
    }
    d.s = r->antialias < 0 ? 0.f : sqrtf(best);
    return d;
}
#endif
