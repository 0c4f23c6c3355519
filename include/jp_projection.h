/* include/jp_projection.h -- camera projections (INTEGRATION.md "Projections"): the orthographic, equirectangular and equidistant-fisheye camera rays, as the
 * device kernels (k_raygen_proj, k_raygen_list_proj, k_other, k_guides, k_camera_rays) and the host entry point jp_projection_rays compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off), and fp32
 * divide / sqrt are the correctly rounded forms on the host and on the device.  The orthographic ray uses only + - * / sqrtf; the equirectangular ray calls
 * sincosf twice and the fisheye once: the host's sincosf on the host, and on the device whatever the including translation unit names in
 * JP_PROJ_SINCOSF_DEVICE (default: JP_LENS_SINCOSF_DEVICE, jp_shading.h: sincos_f, which reproduces the host's libm bit for bit when
 * JpBuildInfo.libm_sincosf != 0).
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_PROJECTION_H
#define JP_PROJECTION_H
#include "jp_lens.h"             /* JP_LENS_FN, JP_LENS_PI, jp_lens_length; jetpbrt_amd.h: JpCamera, JpProjection */

#ifndef JP_PROJ_SINCOSF_DEVICE
#define JP_PROJ_SINCOSF_DEVICE JP_LENS_SINCOSF_DEVICE
#endif

/* Everything a kernel needs, by value: 14 words, made on the host from the uploaded camera (jp_projection_make_plan).
 * ex, ey, ez = right / |right|, up / |up|, front / |front|; scale: the orthographic s; half_fov (radians) and R (pixels): the fisheye's;
 * gamma0: the spread of the ray cone a camera ray starts with (radians per pixel; jp_mipmap.h), which replaces the pinhole's while the projection is in force. */
typedef struct JpProjectionPlan
{
    int32_t kind;
    float   scale, half_fov, R, gamma0;
    float   ex[3], ey[3], ez[3];
} JpProjectionPlan;

JP_LENS_FN void jp_proj_sincos(float x, float* s, float* c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    JP_PROJ_SINCOSF_DEVICE(x, s, c);
#else
    sincosf(x, s, c);
#endif
}

/* the camera ray of the film position (fx, fy) under plan p (kind 1 .. 3); the direction is normalised the way the pinhole's is: one length, three divisions */
JP_LENS_FN void jp_projection_ray(const JpCamera* cam, const JpProjectionPlan* p, float fx, float fy, float origin[3], float dir[3])
{
    float d[3];
    origin[0] = cam->pos[0]; origin[1] = cam->pos[1]; origin[2] = cam->pos[2];
    if (p->kind == JP_PROJ_ORTHOGRAPHIC)
    {
        const float a = fx / cam->res_x - 0.5f, b = 0.5f - fy / cam->res_y;
        const float as = a * p->scale, bs = b * p->scale;
        origin[0] = cam->pos[0] + cam->right[0] * as + cam->up[0] * bs;
        origin[1] = cam->pos[1] + cam->right[1] * as + cam->up[1] * bs;
        origin[2] = cam->pos[2] + cam->right[2] * as + cam->up[2] * bs;
        d[0] = p->ez[0]; d[1] = p->ez[1]; d[2] = p->ez[2];
    }
    else if (p->kind == JP_PROJ_EQUIRECT)
    {
        const float a = fx / cam->res_x - 0.5f, b = 0.5f - fy / cam->res_y;
        const float phi = (2.f * JP_LENS_PI) * a, theta = JP_LENS_PI * b;
        float sp, cp, st, ct;
        jp_proj_sincos(phi, &sp, &cp); jp_proj_sincos(theta, &st, &ct);
        const float wz = ct * cp, wx = ct * sp;
        d[0] = p->ez[0] * wz + p->ex[0] * wx + p->ey[0] * st;
        d[1] = p->ez[1] * wz + p->ex[1] * wx + p->ey[1] * st;
        d[2] = p->ez[2] * wz + p->ex[2] * wx + p->ey[2] * st;
    }
    else
    {
        const float x = fx - cam->res_x / 2.f, y = cam->res_y / 2.f - fy;
        const float rho = sqrtf(x * x + y * y);
        if (rho == 0.f) { d[0] = p->ez[0]; d[1] = p->ez[1]; d[2] = p->ez[2]; }
        else
        {
            const float theta = fminf((rho / p->R) * p->half_fov, JP_LENS_PI);
            float st, ct;
            jp_proj_sincos(theta, &st, &ct);
            const float k = st / rho;
            d[0] = p->ez[0] * ct + (p->ex[0] * x + p->ey[0] * y) * k;
            d[1] = p->ez[1] * ct + (p->ex[1] * x + p->ey[1] * y) * k;
            d[2] = p->ez[2] * ct + (p->ex[2] * x + p->ey[2] * y) * k;
        }
    }
    const float l = jp_lens_length(d);
    dir[0] = d[0] / l; dir[1] = d[1] / l; dir[2] = d[2] / l;
}

/* host side only (plain functions: no device code is generated for them)
 * what jp_set_projection accepts: 0, or the index 1 .. 5 of the first rule broken (struct_bytes, kind, ortho_scale, fov_deg, fit); every field is checked
 * whatever the kind, so a JpProjection is valid or not on its own */
static inline int jp_projection_check(const JpProjection* p)
{
    if (p->struct_bytes < (int32_t)sizeof(JpProjection)) return 1;
    if (p->kind < JP_PROJ_PERSPECTIVE || p->kind > JP_PROJ_FISHEYE) return 2;
    if (!(p->ortho_scale - p->ortho_scale == 0.f) || !(p->ortho_scale >= 0.f)) return 3;
    if (!(p->fov_deg - p->fov_deg == 0.f) || !(p->fov_deg >= 0.f) || !(p->fov_deg <= 360.f)) return 4;
    if (p->fit < JP_FIT_DIAGONAL || p->fit > JP_FIT_HEIGHT) return 5;
    return 0;
}

/* the plan of a checked projection (kind 1 .. 3) on a camera; 0, -1 when right, up or front has no finite positive length (or the resolution is not
 * positive), -2 when the axes of an equirectangular or fisheye camera are not perpendicular (a pairwise |dot| of the unit axes above 1e-3) */
static inline int jp_projection_make_plan(const JpCamera* cam, const JpProjection* pr, JpProjectionPlan* p)
{
    int i;
    const float lr = jp_lens_length(cam->right), lu = jp_lens_length(cam->up), lf = jp_lens_length(cam->front);
    for (i = 0; i < (int)(sizeof(*p) / sizeof(float)); i++) ((float*)p)[i] = 0.f;
    if (!(lr > 0.f && lr - lr == 0.f && lu > 0.f && lu - lu == 0.f && lf > 0.f && lf - lf == 0.f)) return -1;
    if (!(cam->res_x > 0.f && cam->res_y > 0.f)) return -1;
    p->kind = pr->kind;
    for (i = 0; i < 3; i++) { p->ex[i] = cam->right[i] / lr; p->ey[i] = cam->up[i] / lu; p->ez[i] = cam->front[i] / lf; }
    if (pr->kind != JP_PROJ_ORTHOGRAPHIC)
    {
        const float xy = (p->ex[0] * p->ey[0] + p->ex[1] * p->ey[1]) + p->ex[2] * p->ey[2];
        const float xz = (p->ex[0] * p->ez[0] + p->ex[1] * p->ez[1]) + p->ex[2] * p->ez[2];
        const float yz = (p->ey[0] * p->ez[0] + p->ey[1] * p->ez[1]) + p->ey[2] * p->ez[2];
        if (!(fabsf(xy) <= 1e-3f && fabsf(xz) <= 1e-3f && fabsf(yz) <= 1e-3f)) return -2;
    }
    p->scale = pr->ortho_scale == 0.f ? 1.f : pr->ortho_scale;
    {
        const float hx = cam->res_x / 2.f, hy = cam->res_y / 2.f;
        const double fov = pr->fov_deg == 0.f ? 180.0 : (double)pr->fov_deg;
        p->half_fov = (float)(fov * 0.5 * (3.14159265358979323846 / 180.0));
        p->R = pr->fit == JP_FIT_WIDTH ? hx : (pr->fit == JP_FIT_HEIGHT ? hy : sqrtf(hx * hx + hy * hy));
    }
    if (pr->kind == JP_PROJ_EQUIRECT) p->gamma0 = JP_LENS_PI / cam->res_y;
    else if (pr->kind == JP_PROJ_FISHEYE) p->gamma0 = p->half_fov / p->R;
    return 0;
}
#endif
