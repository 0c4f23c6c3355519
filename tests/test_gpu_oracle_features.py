"""Every shading family of the library against the feature oracle (oracle/pt_features.cc; INTEGRATION.md "Feature oracle"), film for film and counter for counter.

A matrix of scene x feature set x kernel row (tests/test_oracle_features_host.py holds the scenes, FAMILIES and CELLS and checks the oracle itself on the CPU).  Every
cell is one render of at most 48 x 32 pixels at 16 spp, depth 6, counter sampler, and asserts
  - the device libm probes report the host's libm reproduced (without that bit equality is not owed),
  - the kernels meant did run: the info structs of every feature, the plan's row (jp_describe_upload under the options in force), JpBuildInfo,
  - the five counters equal the oracle's,
  - the film equals the oracle's bit for bit on every pixel the oracle does not mark undecided (a lookup within its margin of a texel border in acosf / atan2f /
    asinf, which the device takes from its own math library), and the mean per-pixel L2 over ALL pixels is below TOL_L2,
  - every other row of the same scene and feature set rendered so far gave the same bits.
Scenes with a mesh -- all of them -- are rendered on the reference tree, so both sides walk the same tree; one cell runs on the library's own tree under the rule of
test_gpu_parity.assert_film.

The shade_body instantiations the library can launch for these feature sets (jp_render.h shade_choice, jp_shade_launch.h shade_launch), by
<kTab, kPrims, kStage> = (tables in LDS, primitive records in LDS, next-event entries staged), each with kSort on and off:

  family                          TTT        TTF        TFT           TFF        FFF        covered by
  k_shade<..., FeatAll>           zoo_few    zoo        zoo_bulk_few  zoo_bulk   zoo_mats   all
  k_shade_tex                     zoo_few    zoo        zoo_bulk_few  zoo_bulk   zoo_mats   all_tex
  k_shade<T,T,T, sort, FeatLean>  cornell_null (sorted, two-sweep partition), cornell with shade_sort off (unsorted)
  k_shade_lean_one                cornell (sorted, no null material); reserved[0] = 1 on the same scene: k_shade<T,T,T, sort, FeatAll>
  k_shade_pick, _pick_tex         zoo        --         zoo_bulk      --         zoo_mats   pick, pick_tex
  k_shade_env, _env_tex           zoo        --         zoo_bulk      --         zoo_mats   env, env_tex
  k_shade_mis, _mis_tex           zoo        --         zoo_bulk      --         zoo_mats   mis, mis_tex
  k_shade_mis_env, _mis_env_tex   zoo        --         zoo_bulk      --         zoo_mats   mis_env, mis_env_tex
  k_shade_smooth, _tex, _pick, _pick_tex, _env, _env_tex, _mis, _mis_tex, _mis_env, _mis_env_tex<kSort>      zoo with vertex normals (one row: a smooth scene is planned
                                  onto <F,F,F>); with normal maps, sampling records, lens and film state on top: pick_tex_extras (k_shade_smooth_pick_tex behind
                                  k_normal_map_s / k_texel_s), smooth_mis_env_tex_extras; k_raygen<true> and k_resolve_film in both
The side kernel a textured family runs before k_shade*_tex (jp_render.h texel launch: the first that applies), and what of the per-path ray cone it pins
(INTEGRATION.md sections 18, 19; the cone is two floats per path slot that only this kernel reads and writes, through the slot a queued ray carries):

  family                                 side kernel   cone array   rows (scenes), each sorted and unsorted
  *_tex (the ten of the first table)     k_texel       --           as above
  pick_tex_extras, smooth_mis_env_tex_extras   k_texel_s (+ k_normal_map_s)   --   zoo
  all_tex_mip                            k_texel_m     yes          zoo (TTF), zoo_bulk (TFF), zoo_mats (FFF)
  mis_env_tex_mip                        k_texel_m     yes          zoo, zoo_bulk, zoo_mats; zoo_bulk_few in one lane and in three with max_slots = 3 W H
  pick_tex_proc                          k_texel_p     yes (antialiased records alone, no pyramid; bounce_spread from a mipmap state with every mode OFF)
                                                                    zoo, zoo_bulk, zoo_mats; zoo_bulk_few in one lane and in three with max_slots = 3 W H
  pick_tex_proc_off                      k_texel_p     no (every record with antialias off: every width is 0)      zoo, zoo_bulk, zoo_mats
  mis_env_tex_mip_proc                   k_texel_p serving the pyramids too   yes   zoo, zoo_bulk, zoo_mats; zoo generic (reserved[0] = 1); zoo on the library's own tree
  smooth_mis_env_tex_mip_proc_extras     k_texel_p + k_normal_map_s, k_raygen<true>, k_resolve_film   yes   zoo
The mip families put JP_MIP_TRILINEAR on the rectangle image (under a sampling record: its scale enters rho) and on the triangle image (the identity record above level
0), and leave the sphere and disk images JP_MIP_OFF (mixed modes); the records are one of every kind, uv space on triangles, world space on a sphere, one with
antialiasing off, one with a non-identity map, three CHECKER_AA scales (plain word, filtered, 0.5).  The cone meets compaction, the material sort, several workgroup
regions (zoo_bulk: 48 x 32 x 16 slots), lanes with cone arrays of their own, six batches through the same slots with the last one short, the null-material rectangle,
mirror and glass against the widening closures.  tests/test_oracle_features_host.py proves from the oracle's branch statistics that every one of these groups has
at least 2 % of its mip lookups in each of rho <= 1 / two levels / the last level, three values of l, a quarter of the lookups behind a bounce, and every branch of
the records.
  NOT COVERED: a trilinear lookup or a uv-space record on a sphere or a disk (undecided by rule: the uv comes through atan2f / asinf, and every coordinate enters
  the bilinear weights; the footprint areas of the two shapes are pinned ray by ray by jp_mip_probe in tests/test_gpu_mipmap.py), the guides under the cone (pinned
  at the first hit by the guide tests), anisotropic filtering (not in the library).
  NOT COVERED, and not reachable by any scene: the TTF and TFF rows of the eight pick / env / mis families (16 x 2 instances).  plan_scene stages whenever the tables fit
  LDS and the staging area fits next to them, and JP_LIGHTS_POWER_ONE has one shadow plane: 8 KB of staging next to at most 24 KB of tables and records is always within
  the 64 KB, so kStage is false only together with kTab false.  They are compiled and never selected.
  NOT COVERED: the fused k_path schedule (it has no shade_body; every feature here falls back to the per-bounce launches, asserted as fused_last_render 0).
Options: max_slots = 3 W H and lanes on the cone families as the table says; shade_sort on / off in every cell; reserved[0] = 1 (generic) on one family of each group in the zoo; lanes = 1 and lanes = 3 on the same families in zoo_bulk_few
(six row groups of four rows; a scene with a null-material primitive renders in one lane whatever JpOptions.lanes says, and the zoo has one).
"""
import ctypes as C

import numpy as np
import pytest

import jet_pbrt_amd as jp
import harness as H
import test_oracle_features_host as T
from test_gpu_parity import TOL_L2

pytestmark = pytest.mark.gpu
UNSUPPORTED = -5
COUNTERS = ("samples", "closest_rays", "closest_hits", "shadow_rays", "shadow_occluded")


@pytest.fixture(scope="module")
def fctx():
    """a context of this file's own: light sampling, map, estimator, normals, maps, records, lens and film are context state, all of it set by every cell"""
    c = jp.Context(0)
    yield c
    c.close()


def _apply(ctx, st, opts):
    ctx.set_options()
    W, Hh = st["params"].width, st["params"].height
    o = dict(shade_sort=opts.get("shade_sort", 0), lanes=opts.get("lanes", 0), reserved=(C.c_int32 * 8)(1 if opts.get("generic") else 0),
             max_slots={None: 0, "3wh": 3 * W * Hh}[opts.get("max_slots")])     # 3 W H: three of the 16 samples a pixel per batch -- six batches through the same slots, the last one short
    ctx.set_options(**o)
    ctx.set_environment_map(st["rgb"], "y")
    ctx.set_light_sampling(st["mode"])
    ctx.set_vertex_normals(st["vn"])
    ctx.set_normal_maps(st["nmaps"])
    ctx.set_texture_sampling(st["sampling"])
    ctx.set_texture_mipmaps(st["mipmaps"])                          # None clears what an earlier cell left
    ctx.set_texture_procedurals(st["procedurals"])
    ctx.upload(st["sp"], st["textures"])
    ctx.set_estimator(st["est"])
    ctx.set_lens(**T.LENS) if st["lens"] is not None else ctx.set_lens(None)
    ctx.set_film(**T.FILM) if st["film"] is not None else ctx.set_film(None)


def _first_difference(film, ref, und):
    bad = (film.view(np.uint32) != ref.view(np.uint32)).any(-1) & ~und
    if not bad.any():
        return "none"
    y, x = np.argwhere(bad)[0]
    return "pixel (x %d, y %d): device %r, oracle %r; %d decided pixels differ (H.oracle_path_features prints a sample's path)" % (x, y, film[y, x].tolist(), ref[y, x].tolist(), int(bad.sum()))


_device_films = {}


def _check_cell(ctx, variant, family, opts, reference_tree=True):
    fam = T.FAMILIES[family]
    st, ref, cnt, und = T.oracle_of(variant, family, reference_tree)
    lib = jp.hip_lib()
    assert lib.jp_probe_libm_sincosf() != 0 and (lib.jp_probe_libm_xbsdf() & 1) == 1, "the device must reproduce this host's libm (tests/test_libm_exact.py)"
    try:
        _apply(ctx, st, opts)
        film = ctx.render(st["params"])
    except jp.JetPbrtError as e:
        if "status -1" in str(e) or "status -5" in str(e):
            raise
        pytest.exit("the device reported an error (%s): nothing more is started on it" % e, returncode=3)
    # the table the oracle was given is the table on the device
    if fam["mode"] == "power":
        q, alias, pmf = ctx.light_table()
        w, hq, ha, hp = st["features"].table
        assert np.array_equal(q, hq) and np.array_equal(alias, ha) and np.array_equal(pmf, hp)
    c = ctx.counters()
    got = tuple(getattr(c, k) for k in COUNTERS); want = tuple(getattr(cnt, k) for k in COUNTERS)
    l2 = float(np.sqrt(((film - ref) ** 2).sum(-1)).mean())
    decided_equal = (film.view(np.uint32) == ref.view(np.uint32)).all(-1) | und
    print("%s: counters %s (oracle %s); %d undecided pixels, %d of them differ; decided pixels equal: %.5f; mean L2 %.3e" % (
        T.cell_id((variant, family, opts)), got, want, und.sum(), int(((film.view(np.uint32) != ref.view(np.uint32)).any(-1) & und).sum()), decided_equal.mean(), l2))
    # the family meant did run
    bi = ctx.build_info()
    li, ei, mi, ni, ti = ctx.light_info(), ctx.env_info(), ctx.estimator_info(), ctx.normal_info(), ctx.texture_info()
    print("    ran: picked %d mapped %d mis %d textured %d smooth %d (%d smooth triangles) normal-mapped %d sampled %d lens %d film %d; lanes %d, traversal mode %d" % (
        li.picked_last_render, ei.mapped_last_render, mi.mis_last_render, ti.textured_last_render, ni.smooth_last_render, ni.n_smooth_triangles,
        ctx.normal_map_info().mapped_last_render, ctx.texture_sampling_info().sampled_last_render, ctx.lens_info().lens_last_render, ctx.film_info().hdr_last_render,
        bi.lanes_last_render, bi.traversal_mode))
    assert li.picked_last_render == int(fam["mode"] == "power") and ei.mapped_last_render == int(fam["env"]) and mi.mis_last_render == int(fam["est"] == "mis")
    assert ti.textured_last_render == int(fam["tex"])
    assert ni.smooth_last_render == int(fam["smooth"] or fam["nmap"]), (ni.smooth_last_render, ni.n_smooth_triangles)
    if fam["smooth"]:
        assert ni.n_smooth_triangles == int(st["vn"].any(-1).sum()) >= 80
    assert ctx.normal_map_info().mapped_last_render == int(fam["nmap"]) and ctx.texture_sampling_info().sampled_last_render == int(fam["records"])
    assert ctx.lens_info().lens_last_render == int(fam["lens"]) and ctx.film_info().hdr_last_render == int(fam["film"])
    # the side kernel meant did run: k_texel_p with a record (it serves the pyramids too), else k_texel_m with a pyramid, else k_texel_s / k_texel; the cone array exists exactly when a pyramid
    # or an antialiased record does
    mi2, pi = ctx.texture_mipmap_info(), ctx.procedural_info()
    n_rec = len(T.proc_records()) if fam["proc"] else 0
    n_aa = 0 if fam["proc"] != "aa" else sum(1 for r in T.proc_records().values() if r.antialias >= 0)
    print("    side kernel: mip %d (%d pyramids, %d levels), procedural %d (%d records, %d antialiased), cone bytes %d" % (
        mi2.mip_last_render, mi2.n_on, mi2.n_levels, pi.procedural_last_render, pi.n_procedural, pi.n_antialiased, mi2.cone_bytes_device))
    assert (pi.procedural_last_render, pi.n_procedural, pi.n_antialiased) == (int(bool(fam["proc"])), n_rec, n_aa)
    assert (mi2.mip_last_render, mi2.n_on) == (int(fam["mip"]), 2 if fam["mip"] else 0)
    assert (mi2.cone_bytes_device > 0) == bool(fam["mip"] or n_aa > 0)
    if fam["mip"]:
        assert mi2.footprint_scale == np.float32(T.MIP_FOOTPRINT) and mi2.bounce_spread == np.float32(T.MIP_SPREAD)
    assert bi.fused_last_render == 0 and bi.traversal_mode == (5 if reference_tree else bi.traversal_mode)
    if "lanes" in opts:
        assert bi.lanes_last_render == opts["lanes"]
    if reference_tree:
        plan = jp.describe_upload(st["sp"], ctx.get_options(), st["mode"])
        assert plan.shade_sort == int(opts.get("shade_sort", 0) == 1)
        if not (fam["smooth"] or fam["nmap"]):
            assert (plan.tables_in_lds, plan.shade_prims_in_lds, plan.stage_nee) == T.expected_row(variant, fam)
    if reference_tree:
        assert got == want
        assert decided_equal.all(), _first_difference(film, ref, und)
    else:   # the library's own tree (test_gpu_parity.assert_film): a hit in a triangle's fp32 acceptance fringe is found or not depending on the tree
        assert decided_equal.mean() >= 0.999 and got[0] == want[0]
    assert l2 < TOL_L2
    key = (variant, family, reference_tree)
    if key in _device_films:
        assert np.array_equal(_device_films[key].view(np.uint32), film.view(np.uint32)), "the rows of one scene and feature set differ"
    else:
        _device_films[key] = film


@pytest.mark.parametrize("cell", T.CELLS, ids=[T.cell_id(c) for c in T.CELLS])
def test_cell_equals_the_oracle(fctx, cell):
    variant, family, opts = cell
    _check_cell(fctx, variant, family, opts)


def test_a_mesh_row_on_the_default_tree(fctx):
    """the richest family on the library's own tree (no reference semantics): test_gpu_parity.assert_film's rule on the decided pixels"""
    _check_cell(fctx, "zoo", "smooth_mis_env_tex", dict(shade_sort=1), reference_tree=False)


def test_a_cone_row_on_the_default_tree(fctx):
    """pyramids, records and the cone on the library's own tree, under the same rule"""
    _check_cell(fctx, "zoo", "mis_env_tex_mip_proc", dict(shade_sort=1), reference_tree=False)


def test_refused_combinations_stay_refused(fctx):
    """Whitted with smooth triangles, MIS and a map without the light table: JP_ERR_UNSUPPORTED on the device as in the oracle, and the context stays usable"""
    st = T.state_of("zoo", T.FAMILIES["smooth_all"])
    _apply(fctx, st, {})
    film = np.zeros((24, 32, 3), np.float32)
    rw = jp.render_params(32, 24, 1, 3, 1, integrator=jp.JP_INTEGRATOR_WHITTED)
    assert fctx.lib.jp_render(fctx.h, C.byref(rw), film.ctypes.data_as(C.c_void_p)) == UNSUPPORTED
    with pytest.raises(jp.JetPbrtError):
        H.oracle_render_features(st["sp"], rw, st["features"], 2)
    fctx.set_estimator("mis")                                       # the scene was uploaded with JP_LIGHTS_ALL
    assert fctx.lib.jp_render(fctx.h, C.byref(st["params"]), film.ctypes.data_as(C.c_void_p)) == UNSUPPORTED
    fctx.set_estimator(None)
    fctx.set_environment_map(T.env_map_rgb(), "y"); fctx.set_light_sampling(None)
    assert fctx.lib.jp_upload_scene(fctx.h, st["sp"]) == UNSUPPORTED
    fctx.set_environment_map(None)
    _check_cell(fctx, "zoo", "smooth_all", dict(shade_sort=1))
