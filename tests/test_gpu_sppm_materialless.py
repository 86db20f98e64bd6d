"""SPPM in scenes with material-less primitives (GeometricPrimitive(shape) without a material, primitive.jl:1-9) against
oracle/orc_sppm.h, compared as tests/test_gpu_sppm.py compares (M, N, radius, Ld and the visible points bit for bit, ϕ / τ and the
image within the reordering bound).  Camera rays and photons cross such a surface at the same depth with the same β and sampler
dimensions (sppm.jl:218-222, 380-410); a photon deposits at a crossing of depth > 1; shadow rays are still blocked by it.  A call in
which a path crosses more than TRHIP_SPPM_MAX_CROSSINGS of them fails instead of returning an image."""
import os
import re

import numpy as np
import pytest

from test_gpu_sppm import check_pair, run_pair, spot_light

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = int(re.search(r"#define TRHIP_SPPM_MAX_CROSSINGS (\d+)", open(os.path.join(ROOT, "include", "tracehip.h")).read()).group(1))


def ghost_quad(T, p0, p1, p2, p3):
    """Two triangles without a material."""
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    return [T.GeometricPrimitive(t, None) for t in T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, np.float32([p0, p1, p2, p3]))]


def quad_scene(T, y=0.55, x=(0.1, 0.9), z=(-2.9, -2.3), spheres=True):
    """S-cornell with a horizontal material-less quad under the light: camera rays cross it from above, photons on their way down (depth 1)
    and after a bounce off the floor or a sphere (depth > 1, where they deposit)."""
    prims, _ = T.scenes.cornell_primitives(spheres)
    prims += ghost_quad(T, [x[0], y, z[1]], [x[1], y, z[1]], [x[1], y, z[0]], [x[0], y, z[0]])
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


def sheets_scene(T, n):
    """S-cornell without spheres (every camera path ends at its first hit) behind n parallel material-less sheets in front of its open
    side: every camera ray crosses all n, a photon that leaves the box crosses them once and nothing sends it back."""
    prims, _ = T.scenes.cornell_primitives(spheres=False)
    for k in range(n):
        z = -1.05 - 0.1 * k
        prims += ghost_quad(T, [-1.0, -1.0, z], [2.0, -1.0, z], [2.0, 2.5, z], [-1.0, 2.5, z])
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


@pytest.mark.parametrize("batch", [0, 1])
def test_sppm_cornell_with_material_less_quad(T, ob, ctx, batch):
    scene = quad_scene(T)
    cam = T.scenes.cornell_camera(48)
    ctx.set_option("sppm_batch", batch)
    try:
        integ, xyzw, got, ref = run_pair(T, ob, ctx, scene, cam, 0.08, 5, 3, 20000, seed=11)
    finally:
        ctx.set_option("sppm_batch", 0)
    check_pair(T, xyzw, got, ref, 3)
    # the quad is seen through and casts a shadow: more closest-hit rays than the same scene without it, another direct term
    plain = T.SPPMIntegrator(cam, 0.08, 5, 3, 20000, seed=11)
    plain.render(T.scenes.cornell_scene(), ctx)
    assert integ.stats.closest_rays > plain.stats.closest_rays
    assert not np.array_equal(got["Ld"], plain.state()["Ld"])


@pytest.mark.parametrize("hybrid", [1, 0])
def test_sppm_material_less_sphere_spot_light_and_mesh(T, ob, ctx, hybrid):
    """A material-less sphere: every ray through it crosses twice, the second time starting INSIDE it (the certified walk's inside-sphere
    rule, th_trace3c.h; hybrid = 0: every ray on the reference's tree in the reference's order).  Spot light and a BVH with real depth as in
    test_sppm_spot_light_and_mesh.  A ray that leaves the sphere at a grazing angle re-enters it again and again (p + 1e-6 d stays inside within the
    rounding of p: up to hundreds of crossings, about 3.5e-3 / n of the rays through it make more than n), so the call is sized to stay within the
    crossing cap: at 40² x 2 x 30000 photons it does not."""
    base = T.scenes.mesh_scene(24)
    ghost = T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.55, 0.62, -2.55]), False), 0.15, 360.0), None)
    scene = T.Scene([spot_light(T)] + base.lights, T.BVHAccel(list(base.aggregate.primitives) + [ghost], 1))
    cam = T.scenes.cornell_camera(32)
    ctx.set_option("hybrid", hybrid)
    try:
        _, xyzw, got, ref = run_pair(T, ob, ctx, scene, cam, 0.07, 4, 1, 8000, seed=3)
    finally:
        ctx.set_option("hybrid", 1)
    check_pair(T, xyzw, got, ref, 1)


@pytest.mark.parametrize("depth", [2, 4])
def test_sppm_photons_cross_at_depth_one_and_deeper(T, ob, ctx, depth):
    """A material-less quad right under the point light: photons cross it at depth 1 (no deposit) on the way down and at depth > 1 after the
    floor or the ceiling (a deposit each, also at depth == max_depth, where the photon goes on at the same depth)."""
    scene = quad_scene(T, y=0.8, x=(0.3, 0.7), z=(-2.7, -2.3), spheres=False)
    cam = T.scenes.cornell_camera(40)
    _, xyzw, got, ref = run_pair(T, ob, ctx, scene, cam, 0.1, depth, 2, 20000, seed=7)
    check_pair(T, xyzw, got, ref, 2)


def test_sppm_ex_periodic_image_with_material_less_quad(T, ctx):
    """trhip_render_sppm_ex on a scene with a material-less quad: the image handed over after k iterations is a k-iteration call's."""
    scene, cam = quad_scene(T), T.scenes.cornell_camera(40)
    seen = {}
    integ = T.SPPMIntegrator(cam, 0.06, 5, 5, 3000, write_frequency=2, seed=11)
    final = integ.render(scene, ctx, on_write=lambda k, img: seen.__setitem__(k, img.copy())).copy()
    assert sorted(seen) == [2, 4], sorted(seen)
    plain = T.SPPMIntegrator(cam, 0.06, 5, 5, 3000, seed=11).render(scene, ctx)
    assert np.allclose(final, plain, rtol=2e-4, atol=1e-7), "the callback changed the call's result"
    for k, img in seen.items():
        want = T.SPPMIntegrator(cam, 0.06, 5, k, 3000, seed=11).render(scene, ctx)
        assert np.allclose(img, want, rtol=2e-4, atol=1e-7), f"image after {k} iterations: max difference {np.abs(img - want).max()}"
        assert not np.allclose(img, final, rtol=1e-3, atol=1e-6), "an intermediate image equal to the final one proves nothing"


def test_sppm_crossing_cap(T, ob, ctx):
    """K = TRHIP_SPPM_MAX_CROSSINGS sheets render as the oracle renders them; K + 1 make the call fail with a message that names K — also
    under trhip_render_sppm_ex, before any image reaches the callback."""
    cam = T.scenes.cornell_camera(48)
    integ, xyzw, got, ref = run_pair(T, ob, ctx, sheets_scene(T, K), cam, 0.08, 3, 2, 20000, seed=5)
    check_pair(T, xyzw, got, ref, 2)
    assert integ.stats.closest_rays >= 2 * 48 * 48 * (K + 1)  # every camera ray traced K + 1 times
    over = sheets_scene(T, K + 1)
    with pytest.raises(T.TraceHipError, match=rf"more than {K} material-less surfaces \(TRHIP_SPPM_MAX_CROSSINGS = {K}\)") as e:
        T.SPPMIntegrator(cam, 0.08, 3, 2, 20000, seed=5).render(over, ctx)
    assert int(re.search(r"(\d+) camera paths", str(e.value)).group(1)) > 0
    seen = []
    with pytest.raises(T.TraceHipError, match=rf"TRHIP_SPPM_MAX_CROSSINGS = {K}"):
        T.SPPMIntegrator(cam, 0.08, 3, 4, 2000, write_frequency=1, seed=5).render(over, ctx, on_write=lambda k, img: seen.append(k))
    assert seen == []
    # the context renders on afterwards
    T.SPPMIntegrator(cam, 0.08, 3, 1, 2000, seed=5).render(sheets_scene(T, 1), ctx)


def test_sppm_max_depth_limit_with_material_less_primitives(T, ctx):
    """The step loop keeps K steps for crossings: max_depth up to 63 - K."""
    scene, cam = quad_scene(T), T.scenes.cornell_camera(16)
    T.SPPMIntegrator(cam, 0.08, 63 - K, 1, 500, seed=5).render(scene, ctx)
    with pytest.raises(T.TraceHipError, match=f"max_depth must be at most {63 - K}"):
        T.SPPMIntegrator(cam, 0.08, 64 - K, 1, 500, seed=5).render(scene, ctx)


def test_whitted_still_refuses_material_less_primitives(T, ctx):
    """WhittedIntegrator calls a method that does not exist for such a hit (sampler.jl:77-80): the library keeps refusing the scene."""
    with pytest.raises(T.TraceHipError, match="material-less"):
        T.WhittedIntegrator(T.scenes.cornell_camera(16), T.SeededSampler(1), 2).render(quad_scene(T), ctx)
