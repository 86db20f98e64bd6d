"""The oracle's DirectionalLight (oracle/orc_scatter.h: sample_li, directional.jl:39-47) against the composite model of the first vertex (tests/directional_model.py), which
is built from pinned pieces only: depth-1 per-sample radiance of both integrators, bit for bit where the model's BSDF frame is the render's and within 8 ulp elsewhere —
the bar the GPU renders are held to (test_gpu_directional_light.py).  Runs on the CPU, on the reference's own tree."""
import numpy as np
import pytest

import directional_model as dm

SEED = 11


@pytest.mark.parametrize("material", ["matte", "plastic"])
@pytest.mark.parametrize("lights", ["sun", "point_first", "point_after"])
def test_depth1_radiance_matches_the_composite_model(T, ob, material, lights):
    cam = T.scenes.shadows_camera(64)
    for preprocessed in (True, False):
        scene = dm.floor_scene(T, material, lights, preprocessed)
        osc = ob.OracleScene.from_scene(scene)  # with its directional light
        bvh = osc.get_bvh()
        for integrator in ("whitted", "path"):
            what = f"{integrator} {lights} preprocessed={preprocessed} {material}"
            want, exact = dm.direct_terms(T, ob, scene, cam, 4, SEED, integrator, bvh=bvh)
            got = osc.render(cam, integrator, 4, 1, seed=SEED, want_samples=True)[1]
            exact = np.broadcast_to(exact[..., None], want.shape)
            assert exact.mean() > 0.9, what
            assert np.array_equal(np.isnan(got), np.isnan(want)), what
            gi, wi = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
            assert np.array_equal(gi[exact], wi[exact]), f"{what}: bits differ where the model is exact"
            assert np.abs(gi - wi)[~exact & ~np.isnan(want)].max(initial=0) <= 8, f"{what}: more than 8 ulp off where the model's frame is re-normalised"
            if preprocessed and lights == "sun":
                assert (want > 0).any() and (want == 0).any()  # lit floor and shadows


def test_sppm_refuses_a_directional_light(T, ob):
    scene = dm.floor_scene(T, "matte", "point_first", True)
    osc = ob.OracleScene.from_scene(scene)
    with pytest.raises(RuntimeError, match="DirectionalLight"):
        osc.sppm(T.scenes.shadows_camera(16), 0.05, 2, 1, 100, seed=SEED)
