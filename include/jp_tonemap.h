/* include/jp_tonemap.h -- the display transform (INTEGRATION.md "Film"): defaults and validation of a JpToneMap, the exposure scale from a luminance histogram
 * (host, double), and the per-value transform -- exposure, tone curve, Clamp01, the gamma table's byte -- as the device kernel k_display and the host entry point
 * jp_tonemap_host compute it.
 *
 * The per-value arithmetic is fp32 in the order written; the translation units that include this header are compiled without contraction (-ffp-contract=off),
 * and the fp32 divide is the correctly rounded form on the host and on the device.  Only + - * / and comparisons: no library call on the device.
 * Plain C99 / C++ / HIP device code (JP_HD expands to __host__ __device__ under hipcc).
 */
#ifndef JP_TONEMAP_H
#define JP_TONEMAP_H
#include <math.h>
#include <stdint.h>
#include "jetpbrt_amd.h"         /* JpToneMap, JP_CURVE_*, JP_EXPOSURE_*, JP_FILM_BINS */
#include "jp_film.h"             /* jp_film_finite */

#define JP_TONEMAP_KEY      0.18f
#define JP_TONEMAP_WHITE    4.0f
#define JP_TONEMAP_PCT_LOW  0.05f
#define JP_TONEMAP_PCT_HIGH 0.95f
#define JP_TONEMAP_VMAX     1e9f

/* `in` with its defaults filled in -> out; 0 ok, 1 struct_bytes, 2 curve, 3 exposure_mode, 4 ev, 5 key, 6 white, 7 the percentiles */
static inline int jp_tonemap_resolve(const JpToneMap* in, JpToneMap* out)
{
    if (in->struct_bytes < (int32_t)sizeof(JpToneMap)) return 1;
    *out = *in; out->struct_bytes = (int32_t)sizeof(JpToneMap);
    if (in->curve < JP_CURVE_CLAMP || in->curve > JP_CURVE_HABLE) return 2;
    if (in->exposure_mode != JP_EXPOSURE_MANUAL && in->exposure_mode != JP_EXPOSURE_AUTO) return 3;
    if (!jp_film_finite(in->ev)) return 4;
    if (in->key == 0.f) out->key = JP_TONEMAP_KEY;
    if (in->white == 0.f) out->white = JP_TONEMAP_WHITE;
    if (in->pct_low == 0.f) out->pct_low = JP_TONEMAP_PCT_LOW;
    if (in->pct_high == 0.f) out->pct_high = JP_TONEMAP_PCT_HIGH;
    if (!jp_film_finite(out->key) || !(out->key > 0.f)) return 5;
    if (!jp_film_finite(out->white) || !(out->white > 0.f)) return 6;
    if (!jp_film_finite(out->pct_low) || !jp_film_finite(out->pct_high) || !(out->pct_low >= 0.f) || !(out->pct_low < out->pct_high) || !(out->pct_high <= 1.f)) return 7;
    return 0;
}

/* the exposure scale of a resolved tone map; hist: JP_FILM_BINS + 1 counts (the last one, the excluded pixels, is not read); MANUAL reads no histogram */
static inline float jp_tonemap_exposure(const JpToneMap* tm, const uint32_t* hist)
{
    if (tm->exposure_mode == JP_EXPOSURE_MANUAL) return (float)exp2((double)tm->ev);
    double N = 0.0;
    for (int k = 0; k < JP_FILM_BINS; k++) N += (double)hist[k];
    if (!(N > 0.0)) return 1.0f;
    const double lo = (double)tm->pct_low * N, hi = (double)tm->pct_high * N;
    double cum = 0.0, sw = 0.0, sl = 0.0;
    for (int k = 0; k < JP_FILM_BINS; k++)
    {
        const double a = cum, b = cum + (double)hist[k];
        cum = b;
        const double c = (b < hi ? b : hi) - (a > lo ? a : lo);          /* bin k's span of the cumulative count inside [lo, hi] */
        if (!(c > 0.0)) continue;
        const double centre = (1.125 + 0.25 * (double)(k & 3)) * exp2((double)((k >> 2) - 32));
        sw += c; sl += c * log2(centre);
    }
    if (!(sw > 0.0)) return 1.0f;
    const double Lavg = exp2(sl / sw);
    return (float)((double)tm->key / Lavg * exp2((double)tm->ev));
}

#if defined(__HIPCC__)
#define JP_TM_FN static inline JP_HD __attribute__((always_inline))
#else
#define JP_TM_FN static inline
#endif

JP_TM_FN float jp_tm_hable_h(float x) { return ((x * (0.15f * x + 0.05f) + 0.004f) / (x * (0.15f * x + 0.5f) + 0.06f)) - 0.02f / 0.3f; }

/* one value of the film -> y in [0, 1]; w2 = white * white (fp32) */
JP_TM_FN float jp_tm_value(int curve, float w2, float scale, float x)
{
    const float t = x * scale;
    const float v = (t > 0.f) ? (t < JP_TONEMAP_VMAX ? t : JP_TONEMAP_VMAX) : 0.f;
    float y;
    if (curve == JP_CURVE_REINHARD) y = (v * (1.f + v / w2)) / (1.f + v);
    else if (curve == JP_CURVE_ACES) y = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f);
    else if (curve == JP_CURVE_HABLE) y = jp_tm_hable_h(2.f * v) / jp_tm_hable_h(11.2f);
    else y = v;
    return y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
}

/* the number of thresholds <= y: thr holds 256 values, the 255 of jp_gamma_thresholds in ascending order and +infinity */
JP_TM_FN int jp_tm_byte(const float* thr, float y)
{
    int lo = 0;
    for (int step = 128; step > 0; step >>= 1) if (lo + step <= 255 && thr[lo + step - 1] <= y) lo += step;
    return lo;
}

#endif
