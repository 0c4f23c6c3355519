/* include/jp_normals.h -- interpolated shading normals (INTEGRATION.md "Vertex normals"): the barycentrics of a point on a
 * triangle and the shading normal Ns there, as the device kernels (k_normal, k_guides_smooth, k_shading_normal), the host entry
 * point jp_interpolate_normals and the texture lookup (tex_uv, jp_tex.h: the same barycentrics) compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction
 * (-ffp-contract=off), and fp32 divide / sqrt are the correctly rounded forms on the host and on the device.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_NORMALS_H
#define JP_NORMALS_H
#include <math.h>
#include "jp_counter_rng.h"      /* JP_HD */

#define JP_NRM_FLT_MAX 3.402823466e+38f
#if defined(__HIPCC__)
#define JP_NRM_FN static inline JP_HD __attribute__((always_inline))      /* the small arrays of the callers stay in registers */
#else
#define JP_NRM_FN static inline
#endif

/* b1, b2 of a point on a triangle by the normal equations, from e = p1 - p0, f = p2 - p0, g = p - p0 (b0 = 1 - b1 - b2, no clamping); both 0 when den == 0 */
JP_NRM_FN void jp_barycentrics(float ex, float ey, float ez, float fx, float fy, float fz, float gx, float gy, float gz, float* b1, float* b2)
{
    const float d00 = ex * ex + ey * ey + ez * ez, d01 = ex * fx + ey * fy + ez * fz, d11 = fx * fx + fy * fy + fz * fz;
    const float d20 = gx * ex + gy * ey + gz * ez, d21 = gx * fx + gy * fy + gz * fz;
    const float den = d00 * d11 - d01 * d01;
    float a = 0.f, b = 0.f;
    if (den != 0.f) { a = (d11 * d20 - d01 * d21) / den; b = (d00 * d21 - d01 * d20) / den; }
    *b1 = a; *b2 = b;
}

/* Ns at p: m = (b0 n0 + b1 n1) + b2 n2 per component, l2 = dot(m, m); Ng when !(l2 > 0) or l2 is not finite, else m / sqrtf(l2),
 * negated when it lies on the other side of Ng.  vn9 = n0 n1 n2. */
JP_NRM_FN void jp_shading_normal_at(const float p0[3], const float p1[3], const float p2[3], const float ng[3], const float vn9[9], const float p[3], float ns[3])
{
    float b1, b2;
    jp_barycentrics(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], p[0] - p0[0], p[1] - p0[1], p[2] - p0[2], &b1, &b2);
    const float b0 = 1.f - b1 - b2;
    const float mx = (b0 * vn9[0] + b1 * vn9[3]) + b2 * vn9[6];
    const float my = (b0 * vn9[1] + b1 * vn9[4]) + b2 * vn9[7];
    const float mz = (b0 * vn9[2] + b1 * vn9[5]) + b2 * vn9[8];
    const float l2 = mx * mx + my * my + mz * mz;
    if (!(l2 > 0.f && l2 <= JP_NRM_FLT_MAX)) { ns[0] = ng[0]; ns[1] = ng[1]; ns[2] = ng[2]; return; }
    const float l = sqrtf(l2);
    float x = mx / l, y = my / l, z = mz / l;
    if (x * ng[0] + y * ng[1] + z * ng[2] < 0.f) { x = -x; y = -y; z = -z; }
    ns[0] = x; ns[1] = y; ns[2] = z;
}

/* a triangle's nine values as jp_set_vertex_normals accepts them: 0 = flat (nine zeros), 1 = smooth (all finite, 0.81 <= |n|^2 <= 1.21 each), -1 = neither */
JP_NRM_FN int jp_vertex_normals_class(const float vn9[9])
{
    int zeros = 0, k, i;
    for (i = 0; i < 9; i++) { if (!(vn9[i] - vn9[i] == 0.f)) return -1; if (vn9[i] == 0.f) zeros++; }
    if (zeros == 9) return 0;
    for (k = 0; k < 3; k++)
    {
        const float l2 = vn9[3 * k] * vn9[3 * k] + vn9[3 * k + 1] * vn9[3 * k + 1] + vn9[3 * k + 2] * vn9[3 * k + 2];
        if (!(l2 >= 0.81f && l2 <= 1.21f)) return -1;
    }
    return 1;
}
#endif
