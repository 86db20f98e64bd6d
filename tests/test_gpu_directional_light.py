"""DirectionalLight on the MI355X: per-sample radiance against the composite model (tests/directional_model.py), the zero-direction
shadow rays of an un-preprocessed light against the oracle, full-depth renders against the oracle and the reference's tree alone, and SPPM."""

import numpy as np
import pytest

import directional_model as dm

pytestmark = pytest.mark.gpu
SEED = 11


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN pattern differs"
    bad = (bits(a) != bits(b)) & ~na
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_matches_model(got, want, exact, what):
    """Bit for bit where the model's BSDF frame is the render's (directional_model.frame_is_reproducible); within 8 ulp elsewhere."""
    exact = np.broadcast_to(exact[..., None], want.shape)
    assert exact.mean() > 0.9, f"{what}: the model reproduces too few frames"
    assert_bits_equal(np.where(exact, got, 0), np.where(exact, want, 0), what)
    gi, wi = np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(want, np.float32).view(np.int32).astype(np.int64)
    assert np.abs(gi - wi)[~exact].max(initial=0) <= 8, f"{what}: more than 8 ulp off where the model's frame is re-normalised"


CONFIGS = [(lights, pre) for lights in ("sun", "point_first", "point_after") for pre in (True, False)]


@pytest.mark.parametrize("material", ["matte", "plastic"])
@pytest.mark.parametrize("lights,preprocessed", CONFIGS)
@pytest.mark.parametrize("integrator", ["whitted", "path"])
def test_depth1_sample_radiance_matches_the_composite_model(T, ob, ctx, integrator, lights, preprocessed, material):
    scene = dm.floor_scene(T, material, lights, preprocessed)
    cam = T.scenes.shadows_camera(64)
    cls = T.WhittedIntegrator if integrator == "whitted" else T.PathIntegrator
    integ = cls(cam, T.SeededSampler(4, seed=SEED), 1)
    integ.render(scene, ctx)
    got = integ.sample_radiance(scene)
    want, exact = dm.direct_terms(T, ob, scene, cam, 4, SEED, integrator)
    assert_matches_model(got, want, exact, f"{integrator} {lights} preprocessed={preprocessed} {material}")
    if preprocessed and lights == "sun":
        assert (want > 0).any() and (want == 0).any()  # lit floor and shadows


@pytest.mark.parametrize("material", ["matte", "plastic"])
def test_zero_direction_shadow_rays_match_the_oracle(T, ob, ctx, material):
    scene = dm.floor_scene(T, material, "sun", preprocessed=False)
    cam = T.scenes.shadows_camera(64)
    p = dm.hit_points(T, ob, scene, cam, 2, SEED)
    rays = dm.shadow_rays(scene.lights[0], p)
    assert not rays[:, 4:7].any()  # world_radius 0: d is exactly +0
    on_face = np.isin(p[:, 1], [0.0]).sum()
    assert on_face > 100  # origins on the floor: on leaf-box faces, 0 · Inf = NaN in the slab products
    ref = dm.oracle_scene(T, ob, scene).trace_any(rays)[0]
    got = scene.flatten(ctx).trace_any(rays)
    assert np.array_equal(got != 0, ref != 0), f"{int(np.sum((got != 0) != (ref != 0)))} of {rays.shape[0]} differ"


def _film(T, ctx, scene, integrator, depth, spp=4):
    cam = T.scenes.shadows_camera(48)
    cls = T.WhittedIntegrator if integrator == "whitted" else T.PathIntegrator
    integ = cls(cam, T.SeededSampler(spp, seed=SEED), depth)
    return integ.render(scene, ctx).copy()


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("lights,preprocessed", CONFIGS)
@pytest.mark.parametrize("integrator,depth", [("path", 8), ("whitted", 5)])
def test_full_depth_film_equals_the_reference_tree_walk(T, ob, ctx, integrator, depth, lights, preprocessed, special):
    make = lambda: dm.floor_scene(T, "plastic" if special else "matte", lights, preprocessed, special)  # noqa: E731
    a = _film(T, ctx, make(), integrator, depth)
    # ... and the oracle on the committed tree: every vertex of every path under the sun, not the library against itself
    scene = make()
    integ = (T.WhittedIntegrator if integrator == "whitted" else T.PathIntegrator)(T.scenes.shadows_camera(48), T.SeededSampler(4, seed=SEED), depth)
    film = integ.render(scene, ctx).copy()
    osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten(ctx).bvh())
    ref_film, ref_L, ref_st = osc.render(T.scenes.shadows_camera(48), integrator, 4, depth, seed=SEED, want_samples=True)
    assert_bits_equal(integ.sample_radiance(scene), ref_L, f"{integrator} depth {depth}: per-sample radiance vs the oracle")
    assert_bits_equal(film, ref_film, f"{integrator} depth {depth}: film vs the oracle")
    assert_bits_equal(a, ref_film, f"{integrator} depth {depth}: the first run's film vs the oracle")
    assert integ.stats.closest_rays == ref_st.closest_rays and integ.stats.shadow_rays == ref_st.shadow_rays
    b = _film(T, ctx, make(), integrator, depth)
    assert np.isfinite(a).all()
    assert_bits_equal(a, b, "two runs")
    ctx.set_option("bvh_builder", 2)  # the reference's tree alone
    try:
        ref = _film(T, ctx, make(), integrator, depth)
    finally:
        ctx.set_option("bvh_builder", -1)
    assert_bits_equal(a, ref, f"{integrator} depth {depth}: hybrid vs the reference tree")
    if preprocessed:
        assert (a[..., :3] > 0).any()


def test_box_shadow_is_black_at_depth1_and_lit_by_bounces(T, ob, ctx):
    scene = dm.floor_scene(T, "matte", "sun", True)
    cam = T.scenes.shadows_camera(64)
    model, _ = dm.direct_terms(T, ob, scene, cam, 4, SEED, "path")
    samples, rays, osc, prim, geom, order = dm.first_vertex(T, ob, scene, cam, 4, SEED)
    on_floor = (prim >= 0) & (geom[:, 1] == 0)
    shadow = on_floor.reshape(model.shape[:3]) & np.all(model == 0, axis=-1)
    assert shadow.sum() > 20
    integ = T.PathIntegrator(cam, T.SeededSampler(4, seed=SEED), 1)
    integ.render(scene, ctx)
    L1 = integ.sample_radiance(scene)
    assert np.all(L1[shadow] == 0)
    integ = T.PathIntegrator(cam, T.SeededSampler(4, seed=SEED), 8)
    integ.render(scene, ctx)
    L8 = integ.sample_radiance(scene)
    assert (L8[shadow] > 0).any()


def test_sppm_accepted_scene_camera_pass_direct_term(T, ob, ctx):
    scene = dm.floor_scene(T, "matte", "point_first", preprocessed=False)  # a point light, then a zero-power sun: never picked below 2^25 photons
    assert T.api.sppm_directional_pick(scene.lights, 1 * 48 * 48) == -1
    cam = T.scenes.shadows_camera(48)
    integ = T.SPPMIntegrator(cam, 0.05, 1, 1, seed=SEED)
    integ.render(scene, ctx)
    st = integ.state()
    # the camera pass of iteration 1 draws from the stream (seed, pixel, sample 0): one sample per pixel, the direct term without β (A.12)
    want, exact = dm.direct_terms(T, ob, scene, cam, 1, SEED, "path")
    want, exact = want[0], exact[0]
    sb = cam.film.get_sample_bounds()
    x0, y0 = -int(sb.p_min[0]) + 1, -int(sb.p_min[1]) + 1  # film pixel (1, 1) in the sample-pixel grid
    h, w = cam.film.size
    assert_matches_model(st["Ld"], want[y0:y0 + h, x0:x0 + w], exact[y0:y0 + h, x0:x0 + w], "SPPM Ld")
    integ3 = T.SPPMIntegrator(cam, 0.05, 4, 3, seed=SEED)
    a = integ3.render(scene, ctx).copy()
    b = integ3.render(scene, ctx).copy()
    assert np.isfinite(a).all() and np.array_equal(a, b)
    # three iterations at depth 4 against the oracle, which renders a sun that no photon picks (tests/test_gpu_sppm.py's comparison and tolerances)
    from test_gpu_sppm import check_pair, run_pair
    _, xyzw, got, ref = run_pair(T, ob, ctx, scene, cam, 0.05, 4, 3, -1, seed=SEED)
    check_pair(T, xyzw, got, ref, 3)


@pytest.mark.parametrize("lights,preprocessed,photons", [("sun", True, 100), ("sun", False, 100), ("point_after", True, 100), ("point_first", False, 1 << 25)])
def test_sppm_refuses_what_the_mirror_refuses(T, ctx, lights, preprocessed, photons):
    scene = dm.floor_scene(T, "matte", lights, preprocessed)
    cam = T.scenes.shadows_camera(16)
    assert T.api.sppm_directional_pick(scene.lights, photons) >= 0
    integ = T.SPPMIntegrator(cam, 0.05, 2, 1, photons_per_iteration=photons, seed=SEED)
    with pytest.raises(T.TraceHipError, match="sample_le"):
        integ.render(scene, ctx)
