/* include/jp_lens.h -- the thin-lens camera (INTEGRATION.md "Lens"): the lens sample of a disk or polygonal aperture and the camera ray
 * through it, as the device kernels (k_raygen<true>, k_other, k_guides, k_camera_rays) and the host entry point jp_lens_rays compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction
 * (-ffp-contract=off), and fp32 divide / sqrt are the correctly rounded forms on the host and on the device.  The polygon uses only
 * + - * sqrtf; the disk calls sinf / cosf once (concentric mapping): the host's sincosf on the host, and on the device whatever the
 * including translation unit names in JP_LENS_SINCOSF_DEVICE (jp_shading.h: sincos_f, which reproduces the host's libm bit for bit when
 * JpBuildInfo.libm_sincosf != 0).
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_LENS_H
#define JP_LENS_H
#ifndef _GNU_SOURCE
#define _GNU_SOURCE            /* sincosf */
#endif
#include <math.h>
#include "jetpbrt_amd.h"         /* JpCamera, JpLens */
#include "jp_counter_rng.h"      /* JP_HD */

#if defined(__HIPCC__)
#define JP_LENS_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_LENS_FN static inline
#endif

#define JP_LENS_MAX_BLADES 16
#define JP_LENS_PI 3.14159274101257324219f          /* (float)pi, the reference's Pi */

/* Everything a kernel needs, by value: 43 words.  n_verts 0: the disk.  v[k] = (cos, sin)(rotation + 2 pi k / n) for k = 0 .. n, v[n] == v[0]:
 * computed in double on the host and rounded to float, so a polygon needs no trigonometry on the device. */
typedef struct JpLensPlan
{
    float   radius, focus;
    int32_t n_verts;
    float   ex[3], ey[3];                            /* right / |right|, up / |up| */
    float   v[JP_LENS_MAX_BLADES + 1][2];
} JpLensPlan;

/* FSampler's ConcentricSampleDisk (sampling.h:25-50): the one text the BSDF sampling warps and the lens share */
JP_LENS_FN void jp_lens_concentric_disk(float ux, float uy, float* px, float* py)
{
    ux = ux * 2.f - 1.f; uy = uy * 2.f - 1.f;
    if (ux == 0 && uy == 0) { *px = 0; *py = 0; }
    else
    {
        float radius, theta;
        if (fabsf(ux) > fabsf(uy)) { radius = ux; theta = (JP_LENS_PI / 4.0f) * (uy / ux); }
        else { radius = uy; theta = (JP_LENS_PI / 2.0f) - (JP_LENS_PI / 4.0f) * (ux / uy); }
        float st, ct;
#if defined(__HIP_DEVICE_COMPILE__)
        JP_LENS_SINCOSF_DEVICE(theta, &st, &ct);
#else
        sincosf(theta, &st, &ct);
#endif
        *px = ct * radius; *py = st * radius;
    }
}

/* the point on the unit aperture for two draws: uniform in the disk / in the polygon */
JP_LENS_FN void jp_lens_unit_sample(const JpLensPlan* lp, float u0, float u1, float* px, float* py)
{
    if (lp->n_verts == 0) { jp_lens_concentric_disk(u0, u1, px, py); return; }
    const int n = lp->n_verts;
    const float t = u0 * (float)n;
    int k = (int)t; if (k > n - 1) k = n - 1;         /* the triangle (0, v[k], v[k+1]) */
    const float w = t - (float)k;
    const float su = sqrtf(w);
    const float b = u1 * su, c = su - b;
    *px = lp->v[k][0] * b + lp->v[k + 1][0] * c;
    *py = lp->v[k][1] * b + lp->v[k + 1][1] * c;
}

/* the pinhole's direction before normalisation, d0 = front + right * a + up * b: the plane of focus is the set pos + F * d0 */
JP_LENS_FN void jp_lens_d0(const JpCamera* cam, float fx, float fy, float d0[3])
{
    const float a = fx / cam->res_x - 0.5f, b = 0.5f - fy / cam->res_y;
    d0[0] = cam->front[0] + cam->right[0] * a + cam->up[0] * b;
    d0[1] = cam->front[1] + cam->right[1] * a + cam->up[1] * b;
    d0[2] = cam->front[2] + cam->right[2] * a + cam->up[2] * b;
}

JP_LENS_FN float jp_lens_length(const float v[3]) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

/* FCamera::GenerateRay (camera.h:52-58) for the film position (fx, fy): origin pos, direction d0 / |d0| */
JP_LENS_FN void jp_pinhole_ray(const JpCamera* cam, float fx, float fy, float origin[3], float dir[3])
{
    float d0[3]; jp_lens_d0(cam, fx, fy, d0);
    const float l = jp_lens_length(d0);
    origin[0] = cam->pos[0]; origin[1] = cam->pos[1]; origin[2] = cam->pos[2];
    dir[0] = d0[0] / l; dir[1] = d0[1] / l; dir[2] = d0[2] / l;
}

/* the lens ray for the film position (fx, fy) and the two lens draws: from the lens point toward the pinhole ray's point on the plane of focus */
JP_LENS_FN void jp_lens_ray(const JpCamera* cam, const JpLensPlan* lp, float fx, float fy, float u0, float u1, float origin[3], float dir[3])
{
    float px, py; jp_lens_unit_sample(lp, u0, u1, &px, &py);
    const float lx = lp->radius * px, ly = lp->radius * py;
    float d0[3]; jp_lens_d0(cam, fx, fy, d0);
    const float ox = lp->ex[0] * lx + lp->ey[0] * ly, oy = lp->ex[1] * lx + lp->ey[1] * ly, oz = lp->ex[2] * lx + lp->ey[2] * ly;
    origin[0] = cam->pos[0] + ox; origin[1] = cam->pos[1] + oy; origin[2] = cam->pos[2] + oz;
    float q[3];
    q[0] = d0[0] * lp->focus - ox; q[1] = d0[1] * lp->focus - oy; q[2] = d0[2] * lp->focus - oz;   /* (never pos + d0 * F - pos: |pos| would set the error) */
    const float l = jp_lens_length(q);
    dir[0] = q[0] / l; dir[1] = q[1] / l; dir[2] = q[2] / l;
}

/* host side only (plain functions: no device code is generated for them)
 * what jp_set_lens accepts: 0, or the index 1 .. 5 of the first rule broken (struct_bytes, radius, focus_distance, blades, rotation_deg) */
static inline int jp_lens_check(const JpLens* l)
{
    if (l->struct_bytes < (int32_t)sizeof(JpLens)) return 1;
    if (!(l->radius - l->radius == 0.f) || !(l->radius >= 0.f)) return 2;
    if (l->radius > 0.f && (!(l->focus_distance - l->focus_distance == 0.f) || !(l->focus_distance > 0.f))) return 3;
    if (l->blades != 0 && (l->blades < 3 || l->blades > JP_LENS_MAX_BLADES)) return 4;
    if (!(l->rotation_deg - l->rotation_deg == 0.f)) return 5;
    return 0;
}

/* the plan of a checked lens (radius > 0) on a camera; 0, or -1 when right or up has no finite positive length */
static inline int jp_lens_make_plan(const JpCamera* cam, const JpLens* l, JpLensPlan* p)
{
    int k, i;
    const float lr = jp_lens_length(cam->right), lu = jp_lens_length(cam->up);
    for (i = 0; i < (int)(sizeof(*p) / sizeof(float)); i++) ((float*)p)[i] = 0.f;
    if (!(lr > 0.f && lr - lr == 0.f && lu > 0.f && lu - lu == 0.f)) return -1;
    p->radius = l->radius; p->focus = l->focus_distance; p->n_verts = l->blades;
    for (i = 0; i < 3; i++) { p->ex[i] = cam->right[i] / lr; p->ey[i] = cam->up[i] / lu; }
    for (k = 0; k < l->blades; k++)
    {
        const double a = (double)l->rotation_deg * (3.14159265358979323846 / 180.0) + 2.0 * 3.14159265358979323846 * (double)k / (double)l->blades;
        p->v[k][0] = (float)cos(a); p->v[k][1] = (float)sin(a);
    }
    if (l->blades) { p->v[l->blades][0] = p->v[0][0]; p->v[l->blades][1] = p->v[0][1]; }
    return 0;
}
#endif
