/* oracle/pt_features.h -- TEST INFRASTRUCTURE ONLY: the feature state jp_oracle_render_features takes (oracle/pt_features.cc; INTEGRATION.md "Feature oracle").
 * Every field is optional: zero / NULL means "the feature is absent", and with all of them absent the film is jp_oracle_render's, bit for bit.
 * tests/harness.py mirrors this struct in ctypes. */
#ifndef JP_ORACLE_FEATURES_H
#define JP_ORACLE_FEATURES_H
#include "jetpbrt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct JpOracleFeatures {
    int32_t struct_bytes;
    /* light selection: the table as data -- jp_build_light_table's arrays; the oracle restates the pick only */
    int32_t light_mode;                      /* JP_LIGHTS_*                                                                     */
    int32_t n_lights;                        /* entries of q / alias / pmf (== JpScene.n_lights in JP_LIGHTS_POWER_ONE)           */
    int32_t n_env;                           /* entries of env_lights                                                           */
    const float* q; const int32_t* alias; const float* pmf;
    const int32_t* env_lights;               /* the non-black constant environment lights, in light order (JP_LIGHTS_POWER_ONE)  */
    /* environment map as its tables (section 10; jp_build_environment_table's arrays); env_w == 0: no map */
    int32_t env_w, env_h, env_up, env_light; /* size, JP_ENV_UP_*, the map light's index in the scene's light list              */
    const float* env_texel;                  /* 4 per texel: tinted r g b, pdf_t                                                */
    const float* env_q; const int32_t* env_alias;
    const float* env_row_cos;                /* 2 per row: (float)cos(pi r / H), (float)cos(pi (r + 1) / H)                      */
    int32_t estimator;                       /* JP_ESTIMATOR_* (section 11)                                                     */
    int32_t watertight;                      /* jp_oracle_set_watertight for this render                                        */
    const JpVertexNormals* normals;          /* section 12 */
    const JpTextures* textures;              /* section 7  */
    const JpTextureSampling* sampling;       /* section 16 */
    const JpNormalMaps* normal_maps;         /* section 14 */
    const JpLens* lens;                      /* section 13 */
    const JpFilm* film;                      /* section 15 */
    /* appended behind struct_bytes: a caller that passes the shorter struct has none of these */
    const JpTextureMipmaps* mipmaps;         /* section 18: the modes, footprint_scale and bounce_spread (0: the defaults)       */
    int32_t n_mip_chains, pad0;              /* entries of mip_chains (== textures->n_textures, or 0)                            */
    const struct JpOracleMipChain* mip_chains;   /* the pyramids as data, per texture; needed where the mode is TRILINEAR and a material uses the texture */
    const JpTextureProcedurals* procedurals; /* section 19 */
} JpOracleFeatures;

/* the pyramid of one image as jp_build_mip_chain returns it: n_levels sizes and the levels' RGB8 texels in order, level 0 first; n_levels 0: none given */
typedef struct JpOracleMipChain { int32_t n_levels, pad; const int32_t* level_w; const int32_t* level_h; const uint8_t* rgb8; } JpOracleMipChain;

/* What the texture lookups of a render did, per branch of sections 18 and 19; index [0]: lookups at bounce 0, [1]: at bounce >= 1.  The host tests use it to
 * prove that the matrix's scenes reach the code (tests/test_oracle_features_host.py, "reach").
 * mip: lookups on a texture that has a pyramid.  procedural: by kind (JP_PROC_*); all_one: every octave of the record at weight 1; partial: some octave at a weight
 * strictly between 0 and 1; early: the loop stopped at a weight 0 before the record's last octave was evaluated (a lookup can count as partial and early);
 * CHECKER_AA counts in its own three instead.  word_sum: the sum of the side words of every lookup of sections 18 and 19 (order-independent). */
typedef struct JpOracleBranchStats {
    int32_t struct_bytes, pad;
    uint64_t mip_rho_zero[2], mip_rho_le1[2], mip_two_level[2][16] /* by level l */, mip_last_level[2];
    uint64_t proc_all_one[6][2], proc_partial[6][2], proc_early[6][2];
    uint64_t checker_plain[2], checker_filtered[2], checker_half[2];
    uint64_t word_sum[2];
} JpOracleBranchStats;

/* The film and the five counters of `scene` under `params` and `features` (NULL: none).  nthreads as jp_oracle_render takes it; the result does not depend on it.
 * undecided (may be NULL): width * height bytes, 1 where a lookup on one of the pixel's paths came closer to a texel border than the margin
 * (pt_features.cc: lookup_margin) in a function the device takes from its own math library -- there the device may land in the neighbouring texel. */
int jp_oracle_render_features(const JpScene* scene, const JpRenderParams* params, const JpOracleFeatures* features, int nthreads,
                              float* film, JpCounters* counters, uint8_t* undecided);
/* the same render; stats (may be NULL): filled with the lookups' branch counts */
int jp_oracle_render_features_stats(const JpScene* scene, const JpRenderParams* params, const JpOracleFeatures* features, int nthreads,
                                    float* film, JpCounters* counters, uint8_t* undecided, JpOracleBranchStats* stats);
/* debug: sample s of pixel (x, y) alone, every draw, decision and contribution printed to stdout -- with the cone at every hit and rho, l, f or
 * the octave weights of every lookup of sections 18 and 19; out_rgb: the sample's radiance */
int jp_oracle_path_features(const JpScene* scene, const JpRenderParams* params, const JpOracleFeatures* features, int x, int y, int s, float* out_rgb);

#ifdef __cplusplus
}
#endif
#endif
