/* include/jp_normal_map.h -- tangent-space normal maps (INTEGRATION.md "Normal maps"): the decode of a texel, the bilinear lookup, the tangent frame of every
 * shape kind and the perturbed shading normal Ns', as the device kernels (k_normal_map, k_guides_mapped, k_shading_normal_mapped) and the host entry points
 * jp_perturb_normals / jp_triangle_tangents compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction
 * (-ffp-contract=off), and fp32 divide / sqrt are the correctly rounded forms on the host and on the device.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 *
 * Tangent space: x along increasing u, y along increasing v, z along the base normal Nb.  dpdu / dpdv per shape (only their directions matter):
 *   triangle   jp_triangle_tangents below, from the corners and their uvs
 *   rectangle  dpdu = p1 - p0, dpdv = p3 - p0 (the axes of FRectangle::GetUV)
 *   sphere     d = p - centre, GetUV: phi = atan2(d.z, d.x), theta = asin(d.y / r), u = 1 - (phi + pi) / 2pi, v = (theta + pi/2) / pi.  u grows as phi falls
 *              and v as theta grows:  dpdu = (d.z, 0, -d.x),  dpdv = (-d.x d.y, d.x^2 + d.z^2, -d.y d.z)  (d(d)/d(theta) scaled by cos(theta) r^2 > 0).
 *              At the poles dpdu = 0: T degenerates and the hit stays unperturbed.
 *   disk       (s, t, n) = FFrame(normal), l = (dot(s, p - c), dot(t, p - c)), GetUV: u = atan2(l.y, l.x) / 2pi (wrapped to [0, 1)), v = |p - c| / r:
 *              dpdu = -l.y s + l.x t,  dpdv = p - c.  At the centre both are 0: unperturbed.
 */
#ifndef JP_NORMAL_MAP_H
#define JP_NORMAL_MAP_H
#include <math.h>
#include "jp_counter_rng.h"      /* JP_HD */

#define JP_NMAP_FLT_MAX 3.402823466e+38f
#if defined(__HIPCC__)
#define JP_NMAP_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_NMAP_FN static inline
#endif

/* a byte of the map as a tangent-space component: 128 is exactly 0, 255 exactly 1, 0 and 1 both -1 */
JP_NMAP_FN float jp_nmap_decode(unsigned int b)
{
    const float c = ((float)b - 128.f) / 127.f;
    return c < -1.f ? -1.f : c;
}

JP_NMAP_FN int jp_nmap_positive_finite(float x) { return x > 0.f && x <= JP_NMAP_FLT_MAX; }

/* the bilinear lookup between texel centres with clamp addressing; texels: one dword per texel, R | G << 8 | B << 16, row-major, top row first.
 * u, v are clamped to [0, 1] (NaN: 0) and v is flipped. */
JP_NMAP_FN void jp_nmap_lookup(const unsigned int* texels, int w, int h, float u, float v, float m[3])
{
    const float uc = u > 0.f ? (u > 1.f ? 1.f : u) : 0.f;
    const float vc = v > 0.f ? (v > 1.f ? 1.f : v) : 0.f;
    const float x = uc * (float)w - 0.5f, y = (1.f - vc) * (float)h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    int i0 = (int)x0, i1 = (int)x0 + 1, j0 = (int)y0, j1 = (int)y0 + 1;
    i0 = i0 < 0 ? 0 : (i0 > w - 1 ? w - 1 : i0); i1 = i1 < 0 ? 0 : (i1 > w - 1 ? w - 1 : i1);
    j0 = j0 < 0 ? 0 : (j0 > h - 1 ? h - 1 : j0); j1 = j1 < 0 ? 0 : (j1 > h - 1 ? h - 1 : j1);
    const unsigned int t00 = texels[(size_t)j0 * (size_t)w + (size_t)i0], t10 = texels[(size_t)j0 * (size_t)w + (size_t)i1];
    const unsigned int t01 = texels[(size_t)j1 * (size_t)w + (size_t)i0], t11 = texels[(size_t)j1 * (size_t)w + (size_t)i1];
    int k;
    for (k = 0; k < 3; k++)
    {
        const float a = jp_nmap_decode((t00 >> (8 * k)) & 0xffu), b = jp_nmap_decode((t10 >> (8 * k)) & 0xffu);
        const float c = jp_nmap_decode((t01 >> (8 * k)) & 0xffu), d = jp_nmap_decode((t11 >> (8 * k)) & 0xffu);
        const float r0 = a + fx * (b - a), r1 = c + fx * (d - c);
        m[k] = r0 + fy * (r1 - r0);
    }
}

/* Ns' from the tangent-space vector m (before the strength), the base normal nb, the geometric normal ng as k_shade forms it, dpdu and dpdv.
 * Returns 0 ("unperturbed", ns untouched) when mx == my == 0 after the strength, when T's or n's squared length is not positive and finite, or when
 * Ns' does not lie on ng's side. */
JP_NMAP_FN int jp_nmap_apply(const float nb[3], const float ng[3], const float dpdu[3], const float dpdv[3], const float m[3], float strength, float ns[3])
{
    const float mx = m[0] * strength, my = m[1] * strength, mz = m[2];
    if (mx == 0.f && my == 0.f) return 0;
    const float du = nb[0] * dpdu[0] + nb[1] * dpdu[1] + nb[2] * dpdu[2];
    float tx = dpdu[0] - nb[0] * du, ty = dpdu[1] - nb[1] * du, tz = dpdu[2] - nb[2] * du;
    const float t2 = tx * tx + ty * ty + tz * tz;
    if (!jp_nmap_positive_finite(t2)) return 0;
    const float tl = sqrtf(t2);
    tx = tx / tl; ty = ty / tl; tz = tz / tl;
    const float dv = nb[0] * dpdv[0] + nb[1] * dpdv[1] + nb[2] * dpdv[2];
    float bx = dpdv[0] - nb[0] * dv, by = dpdv[1] - nb[1] * dv, bz = dpdv[2] - nb[2] * dv;
    const float tb = tx * bx + ty * by + tz * bz;
    bx = bx - tx * tb; by = by - ty * tb; bz = bz - tz * tb;
    const float b2 = bx * bx + by * by + bz * bz;
    if (jp_nmap_positive_finite(b2)) { const float bl = sqrtf(b2); bx = bx / bl; by = by / bl; bz = bz / bl; }
    else { bx = nb[1] * tz - nb[2] * ty; by = nb[2] * tx - nb[0] * tz; bz = nb[0] * ty - nb[1] * tx; }     /* cross(Nb, T) */
    const float nx = (mx * tx + my * bx) + mz * nb[0], ny = (mx * ty + my * by) + mz * nb[1], nz = (mx * tz + my * bz) + mz * nb[2];
    const float n2 = nx * nx + ny * ny + nz * nz;
    if (!jp_nmap_positive_finite(n2)) return 0;
    const float nl = sqrtf(n2);
    const float x = nx / nl, y = ny / nl, z = nz / nl;
    if (!(x * ng[0] + y * ng[1] + z * ng[2] > 0.f)) return 0;
    ns[0] = x; ns[1] = y; ns[2] = z;
    return 1;
}

/* lookup + apply: the whole definition for one point */
JP_NMAP_FN int jp_perturb_normal(const float nb[3], const float ng[3], const float dpdu[3], const float dpdv[3], float u, float v,
                                 const unsigned int* texels, int w, int h, float strength, float ns[3])
{
    float m[3];
    jp_nmap_lookup(texels, w, h, u, v, m);
    return jp_nmap_apply(nb, ng, dpdu, dpdv, m, strength, ns);
}

/* dpdu, dpdv of a triangle from its corners and uv6 = uv0 uv1 uv2; 0 (both untouched) when the uvs' determinant is 0 or not finite.  The sign of the
 * determinant is folded in, so mirrored uvs give the mirrored dpdv. */
JP_NMAP_FN int jp_triangle_tangents_at(const float p0[3], const float p1[3], const float p2[3], const float uv6[6], float dpdu[3], float dpdv[3])
{
    const float du1 = uv6[2] - uv6[0], dv1 = uv6[3] - uv6[1], du2 = uv6[4] - uv6[0], dv2 = uv6[5] - uv6[1];
    const float det = du1 * dv2 - dv1 * du2;
    int k;
    if (det == 0.f || !(det - det == 0.f)) return 0;
    const float s = det > 0.f ? 1.f : -1.f;
    for (k = 0; k < 3; k++)
    {
        const float e1 = p1[k] - p0[k], e2 = p2[k] - p0[k];
        dpdu[k] = s * (dv2 * e1 - dv1 * e2);
        dpdv[k] = s * (du1 * e2 - du2 * e1);
    }
    return 1;
}

/* sphere: d = p - centre (any positive scale) */
JP_NMAP_FN void jp_sphere_tangents_at(const float d[3], float dpdu[3], float dpdv[3])
{
    dpdu[0] = d[2]; dpdu[1] = 0.f; dpdu[2] = -d[0];
    dpdv[0] = -(d[0] * d[1]); dpdv[1] = d[0] * d[0] + d[2] * d[2]; dpdv[2] = -(d[1] * d[2]);
}

/* disk: s, t the first two axes of FFrame(normal), v0 = p - centre */
JP_NMAP_FN void jp_disk_tangents_at(const float s[3], const float t[3], const float v0[3], float dpdu[3], float dpdv[3])
{
    const float lx = s[0] * v0[0] + s[1] * v0[1] + s[2] * v0[2], ly = t[0] * v0[0] + t[1] * v0[1] + t[2] * v0[2];
    int k;
    for (k = 0; k < 3; k++) { dpdu[k] = t[k] * lx - s[k] * ly; dpdv[k] = v0[k]; }
}
#endif
