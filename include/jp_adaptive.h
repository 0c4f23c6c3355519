/* include/jp_adaptive.h -- adaptive sampling (INTEGRATION.md "Adaptive sampling"): the per-pixel stopping rule on the moments of include/jp_variance.h, as the
 * device kernels (k_resolve_list, k_adapt_select, k_adapt_finish), the host entry point jp_adaptive_samples and the restatement (tests/adaptive_ref.py)
 * compute it.
 *
 * Per pixel of the band shard: n samples taken so far, sum the fp32 rgb sum of those samples in sample-index order (after jp_film_clamp_sample where a film
 * state with sample_clamp > 0 is in force; not scaled), (mean, m2) the moments of jp_var_step with k = the 1-based sample index.
 *   every pixel takes samples 0 .. min_spp - 1; then, until no pixel is active or n == max_spp:
 *     pass(p)   = jp_var_of_mean(m2, n) <= t * t,  t = threshold * max(mean, floor)          (a value that is not finite on either side: pass)
 *     dilate 0:   p stays active iff it was active and does not pass
 *     dilate 1:   p stays active iff it was active and a pixel of its 3 x 3 neighbourhood (clipped to the image and to the band shard; pixels that are
 *                 already inactive count with the state they stopped with) does not pass
 *     active pixels take min(step_spp, max_spp - n) more samples, the next consecutive sample indices
 *   once out, never back in: all active pixels share one n.
 *   film = Clamp01(sum / (float)n) per channel (max(., 0) under hdr), count = n, variance = jp_var_of_mean(m2, n).
 *
 * All arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off).  Only
 * + - * / and comparisons: no library call, no square root (the test compares variances with squared tolerances).
 * Plain C99 / C++ / HIP device code.
 */
#ifndef JP_ADAPTIVE_H
#define JP_ADAPTIVE_H
#include <stdint.h>
#include "jp_variance.h"

#define JP_ADAPT_FN JP_FILM_FN
#define JP_ADAPT_FLOOR_DEFAULT 1e-3f

/* 0 ok, 1 struct_bytes, 2 min_spp, 3 step_spp, 4 max_spp, 5 threshold, 6 floor, 7 dilate.  max_spp 0 (the render's JpRenderParams.spp) is not compared here */
JP_ADAPT_FN int jp_adapt_check(const JpAdaptive* a)
{
    if (a->struct_bytes < (int32_t)sizeof(JpAdaptive)) return 1;
    if (a->min_spp < 2) return 2;
    if (a->step_spp < 1) return 3;
    if (a->max_spp < 0 || (a->max_spp > 0 && a->max_spp < a->min_spp)) return 4;
    if (!jp_film_finite(a->threshold) || !(a->threshold >= 0.f)) return 5;
    if (!jp_film_finite(a->floor) || !(a->floor >= 0.f)) return 6;
    if (a->dilate != 0 && a->dilate != 1) return 7;
    return 0;
}

JP_ADAPT_FN float jp_adapt_floor(float floor_or_zero) { return floor_or_zero > 0.f ? floor_or_zero : JP_ADAPT_FLOOR_DEFAULT; }

/* the test of one pixel after n >= 2 samples; floor: resolved (jp_adapt_floor) */
JP_ADAPT_FN int jp_adapt_pass(float mean, float m2, int32_t n, float threshold, float floor)
{
    const float m = mean > floor ? mean : floor;
    const float t = threshold * m;
    const float tt = t * t;
    const float v = jp_var_of_mean(m2, n);
    if (!jp_film_finite(v) || !jp_film_finite(tt)) return 1;
    return v <= tt ? 1 : 0;
}

/* the samples of the pass after n of max_spp */
JP_ADAPT_FN int32_t jp_adapt_next(int32_t n, int32_t step_spp, int32_t max_spp) { return step_spp < max_spp - n ? step_spp : max_spp - n; }

/* the band shard as the rule sees it: shard-local row r <-> film row y (JpRenderParams: bands of band_rows rows dealt round-robin to shard_count shards) */
typedef struct JpAdaptShard { int32_t width, height, band_rows, shard_index, shard_count; } JpAdaptShard;

JP_ADAPT_FN int32_t jp_adapt_film_row(const JpAdaptShard* s, int32_t r)
{
    const int32_t j = r / s->band_rows;
    return (s->shard_index + j * s->shard_count) * s->band_rows + (r - j * s->band_rows);
}
/* -1: the row lies outside the image or belongs to another shard */
JP_ADAPT_FN int32_t jp_adapt_local_row(const JpAdaptShard* s, int32_t y)
{
    if (y < 0 || y >= s->height) return -1;
    const int32_t b = y / s->band_rows;
    if (b % s->shard_count != s->shard_index) return -1;
    return (b / s->shard_count) * s->band_rows + (y - b * s->band_rows);
}
JP_ADAPT_FN int32_t jp_adapt_local_rows(const JpAdaptShard* s)
{
    const int32_t nbands = (s->height + s->band_rows - 1) / s->band_rows;
    int32_t rows = 0;
    for (int32_t b = s->shard_index; b < nbands; b += s->shard_count) rows += s->band_rows < s->height - b * s->band_rows ? s->band_rows : s->height - b * s->band_rows;
    return rows;
}

/* does shard-local pixel p stay active (it was)?  mean_m2: (mean, m2) pairs, n: the counts, both indexed by shard-local pixel */
JP_ADAPT_FN int jp_adapt_keep(const JpAdaptShard* s, int32_t p, const float* mean_m2, const int32_t* n, int32_t n_stride, float threshold, float floor, int32_t dilate)
{
    if (!dilate) return !jp_adapt_pass(mean_m2[2 * p], mean_m2[2 * p + 1], n[(int64_t)p * n_stride], threshold, floor);
    const int32_t r = p / s->width, x = p - r * s->width, y = jp_adapt_film_row(s, r);
    for (int32_t dy = -1; dy <= 1; dy++)
    {
        const int32_t rr = jp_adapt_local_row(s, y + dy);
        if (rr < 0) continue;
        for (int32_t dx = -1; dx <= 1; dx++)
        {
            const int32_t xx = x + dx;
            if (xx < 0 || xx >= s->width) continue;
            const int32_t q = rr * s->width + xx;
            if (!jp_adapt_pass(mean_m2[2 * q], mean_m2[2 * q + 1], n[(int64_t)q * n_stride], threshold, floor)) return 1;
        }
    }
    return 0;
}

/* one pixel's outputs */
JP_ADAPT_FN void jp_adapt_finish(const float* sum, float m2, int32_t n, int hdr, float* rgb, float* variance)
{
    for (int c = 0; c < 3; c++)
    {
        const float v = sum[c] / (float)n;
        rgb[c] = hdr ? (v > 0.f ? v : 0.f) : (v > 0.f ? (v < 1.f ? v : 1.f) : 0.f);
    }
    *variance = jp_var_of_mean(m2, n);
}

/* Host: the whole loop on caller-supplied samples [max_spp][local pixels][3] of one band shard, without the argument checks (a: checked, max_spp > 0).
 * scratch: jp_adapt_scratch_floats(local pixels) floats.  film / counts / variance: the film's pixel layout (width * height pixels, zero outside the shard),
 * any may be null.  Returns the number of passes run. */
static inline int64_t jp_adapt_scratch_floats(int64_t np) { return 8 * np; }
static inline int32_t jp_adapt_samples(float sample_clamp, int hdr, const JpAdaptive* a, const JpAdaptShard* sh, const float* samples_rgb, float* scratch,
                                       float* film, int32_t* counts, float* variance)
{
    const int32_t np = jp_adapt_local_rows(sh) * sh->width;
    const float floor = jp_adapt_floor(a->floor);
    float* sum = scratch; float* mom = scratch + 3 * (int64_t)np;
    int32_t* n = (int32_t*)(scratch + 5 * (int64_t)np); int32_t* active = (int32_t*)(scratch + 6 * (int64_t)np); int32_t* keep = (int32_t*)(scratch + 7 * (int64_t)np);
    for (int32_t p = 0; p < np; p++) { sum[3 * p] = sum[3 * p + 1] = sum[3 * p + 2] = 0.f; mom[2 * p] = mom[2 * p + 1] = 0.f; n[p] = 0; active[p] = 1; }
    int32_t n_cur = 0, ns = a->min_spp, passes = 0, n_active = np;
    while (n_active > 0)
    {
        for (int32_t p = 0; p < np; p++)
        {
            if (!active[p]) continue;
            for (int32_t s = n_cur; s < n_cur + ns; s++)
            {
                const float* l = samples_rgb + 3 * ((int64_t)s * np + p);
                float r = l[0], g = l[1], b = l[2];
                if (sample_clamp > 0.f) jp_film_clamp_sample(sample_clamp, &r, &g, &b);
                sum[3 * p] = sum[3 * p] + r; sum[3 * p + 1] = sum[3 * p + 1] + g; sum[3 * p + 2] = sum[3 * p + 2] + b;
                jp_var_step(&mom[2 * p], &mom[2 * p + 1], jp_var_luminance(r, g, b), s + 1);
            }
            n[p] = n_cur + ns;
        }
        n_cur += ns; passes++;
        if (n_cur >= a->max_spp) break;
        n_active = 0;
        for (int32_t p = 0; p < np; p++) { keep[p] = active[p] && jp_adapt_keep(sh, p, mom, n, 1, a->threshold, floor, a->dilate); n_active += keep[p]; }
        for (int32_t p = 0; p < np; p++) active[p] = keep[p];
        ns = jp_adapt_next(n_cur, a->step_spp, a->max_spp);
    }
    const int64_t nfilm = (int64_t)sh->width * sh->height;
    if (film) for (int64_t i = 0; i < 3 * nfilm; i++) film[i] = 0.f;
    if (counts) for (int64_t i = 0; i < nfilm; i++) counts[i] = 0;
    if (variance) for (int64_t i = 0; i < nfilm; i++) variance[i] = 0.f;
    for (int32_t p = 0; p < np; p++)
    {
        const int32_t r = p / sh->width, x = p - r * sh->width;
        const int64_t o = (int64_t)jp_adapt_film_row(sh, r) * sh->width + x;
        float rgb[3], v;
        jp_adapt_finish(sum + 3 * p, mom[2 * p + 1], n[p], hdr, rgb, &v);
        if (film) { film[3 * o] = rgb[0]; film[3 * o + 1] = rgb[1]; film[3 * o + 2] = rgb[2]; }
        if (counts) counts[o] = n[p];
        if (variance) variance[o] = v;
    }
    return passes;
}

#endif
