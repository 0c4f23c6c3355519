"""jp_describe_upload against a real upload: what the description says about a scene is what jp_get_build_info reports after jp_upload_scene with the
same options, and the uploaded scene renders (a plan or a view that did not match its tables would show here).  32 x 24 at 4 spp."""
import numpy as np
import pytest

import jet_pbrt_amd as jp
import test_upload_host as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["cornell", "random_1600", "random_1600_certified"])
def test_upload_does_what_the_description_says(name, tmp_path):
    be, sp, _, mode = T.build_case(name, tmp_path)
    ctx = jp.Context(0)
    try:
        ctx.set_light_sampling(mode)
        ctx.upload(sp)
        d = jp.describe_upload(sp, ctx.get_options(), mode)               # the options in force in the context, environment included
        b = ctx.build_info()
        assert b.built_on_device == 0
        assert (b.traversal_mode, b.bvh_nodes, b.bvh_height) == (d.trav_mode, d.bvh_nodes, d.bvh_height)
        assert b.q4_nodes == (d.n_q4 if d.use_q4 else 0) and b.certified_nodes == (d.n_q4 if d.cert else 0)
        assert b.certified_eye_leaves == d.cert_eye_leaves
        if name == "random_1600_certified":
            assert d.cert == 1 and b.certified_nodes > 0
        film = ctx.render(jp.render_params(T.W, T.HH, 4, 5, 1234))
        assert np.isfinite(film).all() and film.mean() > 0.01
    finally:
        ctx.close(); be.close()
