/* include/jp_variance.h -- the per-pixel variance of the film's mean (INTEGRATION.md "Variance"): the running moments of a pixel's sample luminances, as the
 * device kernels (k_resolve_var, k_var_probe) and the host entry point jp_variance_samples and the restatement (tests/variance_ref.py) compute them.
 *
 * Per pixel the samples come in sample-index order, k = 1 .. spp; l is the sample's radiance as it enters the film's sum (after jp_film_clamp_sample where a
 * film state with sample_clamp > 0 is in force):
 *   y    = (0.2126f*l.r + 0.7152f*l.g) + 0.0722f*l.b         (the histogram's luminance; y not finite -> 0)
 *   d    = y - mean;  mean = mean + d / (float)k;  m2 = m2 + d * (y - mean)            (mean = m2 = 0 before k = 1: Welford's recurrence)
 *   variance = (m2 / (float)(spp - 1)) / (float)spp         (the unbiased sample variance over spp: the variance of the pixel's mean luminance)
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off), and the
 * fp32 divide is the correctly rounded form on the host and on the device.  Only + - * / and comparisons: no library call.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_VARIANCE_H
#define JP_VARIANCE_H
#include <stdint.h>
#include "jp_film.h"             /* jp_film_finite, jp_film_clamp_sample */

#define JP_VAR_FN JP_FILM_FN

/* the luminance of one sample as the moments take it */
JP_VAR_FN float jp_var_luminance(float r, float g, float b)
{
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return jp_film_finite(y) ? y : 0.f;
}

/* sample k (1-based) of a pixel enters its moments */
JP_VAR_FN void jp_var_step(float* mean, float* m2, float y, int32_t k)
{
    const float d = y - *mean;
    const float m = *mean + d / (float)k;
    *m2 = *m2 + d * (y - m);
    *mean = m;
}

/* the variance of the mean of spp >= 2 samples */
JP_VAR_FN float jp_var_of_mean(float m2, int32_t spp) { return (m2 / (float)(spp - 1)) / (float)spp; }

/* jp_variance_samples without its argument checks: samples_rgb [spp][n_pixels][3]; sample_clamp 0: no clamp; variance_out / mean_out: n_pixels floats, either may be null */
JP_VAR_FN void jp_var_samples(float sample_clamp, int32_t spp, int64_t n_pixels, const float* samples_rgb, float* variance_out, float* mean_out)
{
    for (int64_t p = 0; p < n_pixels; p++)
    {
        float mean = 0.f, m2 = 0.f;
        for (int32_t s = 0; s < spp; s++)
        {
            const float* l = samples_rgb + 3 * ((int64_t)s * n_pixels + p);
            float r = l[0], g = l[1], b = l[2];
            if (sample_clamp > 0.f) jp_film_clamp_sample(sample_clamp, &r, &g, &b);
            jp_var_step(&mean, &m2, jp_var_luminance(r, g, b), s + 1);
        }
        if (variance_out) variance_out[p] = jp_var_of_mean(m2, spp);
        if (mean_out) mean_out[p] = mean;
    }
}

#endif
