/* include/jp_film.h -- the film state (INTEGRATION.md "Film"): the per-sample firefly clamp of jp_set_film and the luminance bin of jp_film_histogram, as
 * the device kernels (k_resolve_film, k_film_hist) and the host entry points jp_film_samples and the restatements compute them.
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off), and the
 * fp32 divide is the correctly rounded form on the host and on the device.  Only + * / and comparisons: no library call.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_FILM_H
#define JP_FILM_H
#include <stdint.h>
#include <string.h>
#include "jetpbrt_amd.h"         /* JpFilm, JP_FILM_BINS */
#include "jp_counter_rng.h"      /* JP_HD */

#if defined(__HIPCC__)
#define JP_FILM_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_FILM_FN static inline
#endif

JP_FILM_FN uint32_t jp_film_bits(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u; memcpy(&u, &x, 4); return u;
#endif
}
/* neither an infinity nor a NaN: the exponent field is not all ones */
JP_FILM_FN int jp_film_finite(float x) { return (jp_film_bits(x) & 0x7f800000u) != 0x7f800000u; }

/* 0 ok, 1 struct_bytes, 2 hdr, 3 sample_clamp */
JP_FILM_FN int jp_film_check(const JpFilm* f)
{
    if (f->struct_bytes < (int32_t)sizeof(JpFilm)) return 1;
    if (f->hdr != 0 && f->hdr != 1) return 2;
    if (!jp_film_finite(f->sample_clamp) || !(f->sample_clamp >= 0.f)) return 3;
    return 0;
}

/* jp_set_film's sample_clamp c > 0 on one sample's radiance, in place */
JP_FILM_FN void jp_film_clamp_sample(float c, float* r, float* g, float* b)
{
    const float lr = *r, lg = *g, lb = *b;
    if (!jp_film_finite(lr) || !jp_film_finite(lg) || !jp_film_finite(lb)) { *r = 0.f; *g = 0.f; *b = 0.f; return; }
    float m = lr < lg ? lg : lr;
    m = m < lb ? lb : m;
    if (m > c)
    {
        const float k = c / m;
        *r = lr * k; *g = lg * k; *b = lb * k;
    }
}

/* the bin of one pixel: 0 .. JP_FILM_BINS - 1, or JP_FILM_BINS for a pixel the histogram excludes */
JP_FILM_FN int jp_film_bin(float r, float g, float b)
{
    const float Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    if (!(Y > 0.f) || !jp_film_finite(Y)) return JP_FILM_BINS;
    const int k = (int)(jp_film_bits(Y) >> 21) - 380;
    return k < 0 ? 0 : (k > JP_FILM_BINS - 1 ? JP_FILM_BINS - 1 : k);
}

#endif
