#!/usr/bin/env python3
"""Golden for tests/test_oracle_vs_reference.py and the larger gamma_encoding sample of tests/test_host_and_abi.py: the
UNMODIFIED reference (oracle/_ref/libjp_ref.so) renders every configuration those tests list -- FPathIntegratorIteration on
both samplers and its serial whole-frame path, the procedural bunny at two resolutions, random scenes, FWhittedIntegrator
and FDebugIntegrator -- and encodes 250,000 values through gamma_encoding (film.h:24).  The fixture keeps the raw fp32 films,
the reference's primitive / light counts, the procedural meshes the bunny renders read (numpy's sin / cos may differ in the
last bit between hosts; the golden must not), and the SHA-256 of the gamma bytes (data only).
Run where the reference build exists (oracle/ref_build):  python tests/golden/make_golden_vs_reference.py"""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import harness as H  # noqa: E402
import test_host_and_abi  # noqa: E402
import test_oracle_vs_reference as T  # noqa: E402


def main():
    assert H.have_ref()
    out = {}
    for name, W, Hh, spp, depth, seed in T.EQ_CASES:
        H.libc_srand(1)
        rb = H.SCENES[name](H.RefBackend(name), W, Hh)
        key = T.eq_key(name, W, Hh, spp, depth, seed)
        for mode in (0, 1):
            out["%s_m%d" % (key, mode)] = rb.render(W, Hh, spp, depth, mode, seed, 4)
        out[key + "_serial"] = rb.render(W, Hh, 1, depth, 0, seed, 0)          # the serial whole-frame path of Render (numthreads < 1)
        rb.close()
    d = tempfile.mkdtemp(prefix="jp_golden_")
    for nlon, nlat in T.SWEEP:
        key = "sweep_%dx%d" % (nlon, nlat)
        v, f = H.scenes.bunny_mesh(nlon, nlat)
        out[key + "_verts"] = np.asarray(v, np.float32); out[key + "_faces"] = np.asarray(f, np.int32)
        obj = H.scenes.write_obj(os.path.join(d, key + ".obj"), out[key + "_verts"], out[key + "_faces"])
        H.libc_srand(1)
        rb = H.scenes.build_bunny(H.RefBackend("b"), T.SWEEP_W, T.SWEEP_H, obj_path=obj)
        out[key + "_nprims"] = np.int64(rb.num_primitives())
        out[key] = rb.render(T.SWEEP_W, T.SWEEP_H, 2, 5, 1, 1234, 4)
        rb.close()
    for seed in T.RANDOM_SEEDS:
        H.libc_srand(1)
        rb = H.build_random_scene(H.RefBackend("r"), T.RANDOM_W, T.RANDOM_H, seed, tmpdir=d)
        out["random_%d_counts" % seed] = np.array([rb.num_primitives(), rb.num_lights()], np.int64)
        for mode in (0, 1):
            out["random_%d_m%d" % (seed, mode)] = rb.render(T.RANDOM_W, T.RANDOM_H, T.RANDOM_SPP, 5, mode, 77, 4)
        rb.close()
    for name in T.OTHER_SCENES:
        for kind in T.OTHER_KINDS:
            H.libc_srand(1)
            rb = H.SCENES[name](H.RefBackend(name), T.OTHER_W, T.OTHER_H)
            for depth in (5, 2):
                out["other_%s_k%d_d%d" % (name, kind, depth)] = rb.render_other(kind, T.OTHER_W, T.OTHER_H, T.OTHER_SPP, depth, 55)
            rb.close()
    xr = test_host_and_abi.gamma_sample()
    yr = np.zeros(xr.size, np.uint8)
    H.ref_lib().ref_gamma_encode(H.ptr(xr), xr.size, H.ptr(yr))
    out["gamma_sha256"] = np.array(hashlib.sha256(yr.tobytes()).hexdigest())
    np.savez_compressed(os.path.join(HERE, "vs_reference.npz"), **out)
    print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "vs_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
