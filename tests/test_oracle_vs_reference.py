"""CPU suite, part 2: the restatement against the compiled reference on configurations the 48x48 goldens do not hold.  The
reference's films are data under tests/golden/vs_reference.npz (tests/golden/make_golden_vs_reference.py renders them with the
UNMODIFIED reference, oracle/_ref/libjp_ref.so); the oracle renders the same configurations here and must equal them bit for bit."""
import os

import numpy as np
import pytest

import harness as Hm

EQ_CASES = [
    ("cornell", 40, 30, 3, 5, 7), ("cornell_lambert", 33, 47, 2, 2, 99), ("bunny_small", 64, 40, 4, 5, 1234),
    ("misc", 56, 56, 6, 8, 5), ("cornell", 16, 16, 32, 0, 3), ("misc", 20, 61, 5, 1, 11), ("lights", 48, 40, 4, 5, 21),
    ("disks", 64, 64, 8, 5, 31), ("disks", 37, 53, 3, 2, 8)]
SWEEP, SWEEP_W, SWEEP_H = ((40, 30), (61, 44)), 48, 36
RANDOM_SEEDS, RANDOM_W, RANDOM_H, RANDOM_SPP = [1, 2, 3], 40, 32, 4
OTHER_SCENES, OTHER_KINDS, OTHER_W, OTHER_H, OTHER_SPP = ["cornell", "misc", "lights", "disks", "bunny_small"], [1, 2], 40, 36, 3


def eq_key(name, W, Hh, spp, depth, seed):
    return "eq_%s_%dx%d_%dspp_d%d_s%d" % (name, W, Hh, spp, depth, seed)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(Hm.GOLDEN, "vs_reference.npz"))


def _equal(fr, fo):
    return np.array_equal(fr.view(np.uint32), fo.view(np.uint32))


@pytest.mark.parametrize("name,W,Hh,spp,depth,seed", EQ_CASES)
def test_live_reference_equality(H, ref, name, W, Hh, spp, depth, seed):
    hb = H.SCENES[name](H.scenes.HostBackend(name), W, Hh)
    sp = hb.flatten()
    key = eq_key(name, W, Hh, spp, depth, seed)
    for mode in (0, 1):
        fr = ref["%s_m%d" % (key, mode)]
        fo, _ = H.oracle_render(sp, H.jp.render_params(W, Hh, spp, depth, seed, mode), 4)
        assert _equal(fr, fo), (name, mode, float(np.abs(fr - fo).max()))
    # the serial whole-frame path of Render (numthreads < 1)
    fo, _ = H.oracle_render(sp, H.jp.render_params(W, Hh, 1, depth, seed, 0), 0)
    assert _equal(ref[key + "_serial"], fo)


def test_bunny_mesh_resolution_sweep(H, ref, tmp_path):
    """larger procedural meshes: reference ingest (obj_loader) vs own OBJ reader + topology-independent hits.  The meshes are the
    golden's (the reference read exactly these vertices), written to OBJ here as the scene builder writes them."""
    for nlon, nlat in SWEEP:
        key = "sweep_%dx%d" % (nlon, nlat)
        obj = H.scenes.write_obj(str(tmp_path / (key + ".obj")), ref[key + "_verts"], ref[key + "_faces"])
        hb = H.scenes.build_bunny(H.scenes.HostBackend("b"), SWEEP_W, SWEEP_H, obj_path=obj)
        assert int(ref[key + "_nprims"]) == hb.num_primitives() == 4 * 2 * nlon * (nlat - 1) + 2
        fo, _ = H.oracle_render(hb.flatten(), H.jp.render_params(SWEEP_W, SWEEP_H, 2, 5, 1234, 1), 4)
        assert _equal(ref[key], fo)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_scenes_live_reference(H, ref, tmp_path, seed):
    """random soups + all shape kinds as lights + all materials: the restatement stays bit-identical to the reference"""
    hb = H.build_random_scene(H.scenes.HostBackend("r"), RANDOM_W, RANDOM_H, seed, tmpdir=str(tmp_path))
    nprims, nlights = (int(v) for v in ref["random_%d_counts" % seed])
    assert nprims == hb.num_primitives() and nlights == hb.num_lights() == 5
    for mode in (0, 1):
        fr = ref["random_%d_m%d" % (seed, mode)]
        fo, _ = H.oracle_render(hb.flatten(), H.jp.render_params(RANDOM_W, RANDOM_H, RANDOM_SPP, 5, 77, mode), 4)
        assert np.isfinite(fr).all()
        assert _equal(fr, fo), float(np.abs(fr - fo).max())


@pytest.mark.parametrize("name", OTHER_SCENES)
@pytest.mark.parametrize("kind", OTHER_KINDS)
def test_other_integrators_live_reference(H, ref, name, kind):
    """FWhittedIntegrator (integrator.cc:115-220: two branches at every mirror, draws in depth-first order) and
    FDebugIntegrator (integrator.h:44-58): the restatement is bit-identical to the compiled reference"""
    hb = H.SCENES[name](H.scenes.HostBackend(name), OTHER_W, OTHER_H)
    for depth in (5, 2):
        fr = ref["other_%s_k%d_d%d" % (name, kind, depth)]
        fo, _ = H.oracle_render(hb.flatten(), H.jp.render_params(OTHER_W, OTHER_H, OTHER_SPP, depth, 55, integrator=kind), 0)
        assert np.isfinite(fr).all()
        assert _equal(fr, fo), (name, kind, depth, float(np.abs(fr - fo).max()))
