"""Relit views (Scene.with_lights, trhip_scene_relight) on the MI355X: a view shares its base's committed geometry, commits only its lights, and renders bit for
bit what a fresh commit of the same primitives with those lights renders (and what the oracle renders on the same tree)."""

import ctypes as C

import numpy as np
import pytest

import directional_model as dm
import test_gpu_sppm as sppm

pytestmark = pytest.mark.gpu
SEED = 7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} values differ, first at {np.argwhere(bad)[0]}"


def point(T, pos=(0.5, 0.9, -2.5), intensity=2.5):
    return T.PointLight(T.translate(list(pos)), T.RGBSpectrum(intensity))


def frame(T, ctx, scene, cam, integrator, depth, spp=2):
    cls = T.WhittedIntegrator if integrator == "whitted" else T.PathIntegrator
    integ = cls(cam, T.SeededSampler(spp, seed=SEED), depth)
    film = integ.render(scene, ctx).copy()
    return film, integ.sample_radiance(scene).copy()


def check_relit(T, ob, ctx, base, lights, cam, integrator, depth, preprocess=False):
    """base.with_lights(lights) against a fresh Scene(lights, base.aggregate) and against the oracle on the view's tree."""
    relit = base.with_lights(lights)
    fresh = T.Scene(lights, base.aggregate)
    if preprocess:
        for l in lights:
            T.preprocess(l, relit)
    got = frame(T, ctx, relit, cam, integrator, depth)
    want = frame(T, ctx, fresh, cam, integrator, depth)
    what = f"{integrator}, {len(lights)} lights"
    assert_bits_equal(got[0], want[0], f"{what}: film, relit vs fresh commit")
    assert_bits_equal(got[1], want[1], f"{what}: per-sample radiance, relit vs fresh commit")
    fv, fb, ff = relit.flatten(ctx), base.flatten(ctx), fresh.flatten(ctx)
    assert fv.geometry_id == fb.geometry_id != ff.geometry_id
    assert fv.bvh_mode() == fb.bvh_mode()
    osc = ob.OracleScene.from_scene(relit, bvh=fv.bvh())  # a DirectionalLight goes over with its fields as they stand, preprocessed or not
    ref_xyzw, ref_L, _ = osc.render(cam, integrator, 2, depth, seed=SEED, want_samples=True)
    assert_bits_equal(got[1], ref_L, f"{what}: per-sample radiance, relit vs oracle")
    assert_bits_equal(got[0], ref_xyzw, f"{what}: film, relit vs oracle")
    return got


@pytest.mark.parametrize("builder", [-1, 2, 0])
@pytest.mark.parametrize("integrator,depth", [("path", 5), ("whitted", 5)])
def test_cornell_light_changes(T, ob, ctx, builder, integrator, depth):
    """S-cornell under the default hybrid commit (the accelerator is one leaf: its any-hit order is the light stage's), the reference's tree alone and the library's
    one-leaf tree, the option set BEFORE the base commit."""
    ctx.set_option("bvh_builder", builder)
    try:
        base = T.scenes.cornell_scene()
        cam = T.scenes.cornell_camera(32)
        base_film = frame(T, ctx, base, cam, integrator, depth)
        mode = base.flatten(ctx).bvh_mode()[0]
        assert mode == {-1: 2, 2: 1, 0: 0}[builder]
        spot = sppm.spot_light(T)
        sun = dm.sun(T)
        check_relit(T, ob, ctx, base, [spot], cam, integrator, depth)  # point -> spot
        check_relit(T, ob, ctx, base, [point(T, (0.3, 0.9, -2.2), 1.5), spot], cam, integrator, depth)  # point -> point + spot
        lit = check_relit(T, ob, ctx, base, [point(T), sun], cam, integrator, depth, preprocess=True)  # a DirectionalLight: the DIRL kernels
        assert not np.array_equal(lit[0], base_film[0])
        back = check_relit(T, ob, ctx, base, base.lights, cam, integrator, depth)  # ... and back without it
        assert_bits_equal(back[0], base_film[0], "relit to the base's own lights vs the base")
        dark = check_relit(T, ob, ctx, base, [], cam, integrator, depth)  # no lights at all
        assert np.isfinite(dark[0]).all()
    finally:
        ctx.set_option("bvh_builder", -1)


@pytest.mark.parametrize("which", ["mesh_occluders", "one_leaf"])
def test_light_ordered_paths(T, ob, ctx, which):
    """The paths whose any-hit orders the light stage recomputes: the largest-triangle pre-pass (mesh_scene(40): its walls) and a one-leaf scene."""
    if which == "mesh_occluders":
        base, cam = T.scenes.mesh_scene(40), T.scenes.cornell_camera(32)
    else:
        base, cam = T.scenes.shadows_scene(), T.scenes.shadows_camera(32)
        ctx.set_option("bvh_builder", 0)  # the library's tree: one leaf (tiny_scene_prims)
    try:
        frame(T, ctx, base, cam, "path", 5)
        lights = [[sppm.spot_light(T)], [point(T, (0.2, 0.95, -2.1), 1.5), sppm.spot_light(T)], [point(T, (0.8, 0.5, -2.0), 2.0)]]
        for ls in lights:
            check_relit(T, ob, ctx, base, ls, cam, "path", 5)
    finally:
        ctx.set_option("bvh_builder", -1)


def test_sppm(T, ob, ctx):
    """Two lights (sample_discrete over their power) on a relit Cornell box against a fresh commit and the oracle; a view whose photon pass could pick a DirectionalLight
    is refused as a fresh commit is; relit back, it renders."""
    base = T.scenes.cornell_scene()
    cam = T.scenes.cornell_camera(48)
    iters, photons = 3, 20000
    base.flatten(ctx)
    lights = [point(T, (0.3, 0.9, -2.2), 1.5), sppm.spot_light(T)]
    relit = base.with_lights(lights)
    _, xyzw, got, ref = sppm.run_pair(T, ob, ctx, relit, cam, 0.08, 5, iters, photons, seed=11)
    sppm.check_pair(T, xyzw, got, ref, iters)
    fresh = T.Scene(lights, base.aggregate)
    _, xyzw_f, got_f, _ = sppm.run_pair(T, ob, ctx, fresh, cam, 0.08, 5, iters, photons, seed=11)
    sppm.check_pair(T, xyzw_f, got_f, ref, iters)
    for k in ("M", "N", "radius", "Ld", "vp_p", "vp_beta"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(got_f[k]).view(np.uint8)), f"{k}: relit vs fresh commit"
    assert relit.flatten(ctx).geometry_id == base.flatten(ctx).geometry_id
    sun = dm.sun(T)
    sunny = base.with_lights([sun])
    T.preprocess(sun, sunny)
    assert T.api.sppm_directional_pick(sunny.lights, photons) >= 0
    for sc in (sunny, T.Scene([sun], base.aggregate)):
        with pytest.raises(T.TraceHipError, match="sample_le"):
            T.SPPMIntegrator(cam, 0.08, 5, 1, photons, seed=11).render(sc, ctx)
    again = base.with_lights(lights)
    _, xyzw2, got2, _ = sppm.run_pair(T, ob, ctx, again, cam, 0.08, 5, iters, photons, seed=11)
    sppm.check_pair(T, xyzw2, got2, ref, iters)


def _extra_triangle(T, material):
    """One big triangle across the Cornell box, in world space (identity ShapeCore), as api objects and as the raw arrays of trhip_scene_add_triangles."""
    verts = np.float32([[0.1, 0.05, -2.2], [0.9, 0.05, -2.2], [0.5, 0.6, -2.9]])
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    tri = T.create_triangle_mesh(core, 1, np.array([1, 2, 3], np.uint32), 3, verts.tolist())[0]
    return T.GeometricPrimitive(tri, material), verts


def test_sharing_and_lifetime(T, ob, ctx):
    L = T.lib()
    base = T.scenes.cornell_scene()
    cam = T.scenes.cornell_camera(32)
    fb = base.flatten(ctx)
    lights = [sppm.spot_light(T)]
    relit = base.with_lights(lights)
    twice = relit.with_lights([point(T, (0.3, 0.9, -2.2), 1.5)])
    fresh = T.Scene(lights, base.aggregate)
    ids = [s.flatten(ctx).geometry_id for s in (base, relit, twice, fresh)]
    assert ids[0] == ids[1] == ids[2] != ids[3] and ids[0] != 0, ids
    want_relit, want_twice = frame(T, ctx, fresh, cam, "path", 5), frame(T, ctx, T.Scene(twice.lights, base.aggregate), cam, "path", 5)
    assert_bits_equal(frame(T, ctx, twice, cam, "path", 5)[0], want_twice[0], "a view of a view")
    # free the base: its views keep the geometry
    fb.free()
    got = frame(T, ctx, relit, cam, "path", 5)
    assert_bits_equal(got[0], want_relit[0], "film after the base was freed")
    assert_bits_equal(got[1], want_relit[1], "radiance after the base was freed")
    assert_bits_equal(frame(T, ctx, twice, cam, "path", 5)[0], want_twice[0], "a view of a view after the base was freed")

    # add a primitive to a base and commit it again: the base gets new geometry, the view keeps the old
    base = T.scenes.cornell_scene()
    fb = base.flatten(ctx)
    relit = base.with_lights(lights)
    fv = relit.flatten(ctx)
    old_id = fb.geometry_id
    mat0 = T.api.splice_nested(base.aggregate.primitives)[0].material
    extra, verts = _extra_triangle(T, mat0)
    idx, mats = np.array([1, 2, 3], np.uint32), np.zeros(1, np.uint32)  # material 0: the first one the base registered (mat0)
    ctx.check(L.trhip_scene_add_triangles(fb._h, T._ffi.fptr(verts), 3, T._ffi.u32ptr(idx), 1, None, T._ffi.u32ptr(mats), 0, None))
    ctx.check(L.trhip_scene_commit(fb._h, 1))
    assert fb.geometry_id not in (0, old_id) and fv.geometry_id == old_id
    got = frame(T, ctx, relit, cam, "path", 5)
    assert_bits_equal(got[0], want_relit[0], "the old view after its base grew")
    grown = T.Scene(base.lights, T.BVHAccel(list(base.aggregate.primitives) + [extra], 1))
    assert_bits_equal(frame(T, ctx, base, cam, "path", 5)[0], frame(T, ctx, grown, cam, "path", 5)[0], "the grown base vs a fresh commit of the grown scene")
    assert fb.bvh()[3].size == fv.bvh()[3].size + 1

    # an option changed after the base commit does not apply to its views: they keep the base's trees
    base = T.scenes.mesh_scene(16)
    fb = base.flatten(ctx)
    assert fb.bvh_mode()[0] == 2
    ctx.set_option("bvh_builder", 0)
    try:
        fv = base.with_lights(lights).flatten(ctx)
        assert fv.bvh_mode() == fb.bvh_mode() and fv.bvh_note() == fb.bvh_note()
        for x, y in zip(fv.bvh(), fb.bvh()):
            assert np.array_equal(x, y)
        for x, y in zip(fv.accelerator(), fb.accelerator()):
            assert np.array_equal(x, y)
        assert T.Scene(lights, base.aggregate).flatten(ctx).bvh_mode()[0] == 0
    finally:
        ctx.set_option("bvh_builder", -1)


def test_refusals(T, ob, ctx):
    L = T.lib()
    base = T.scenes.cornell_scene()
    cam = T.scenes.cornell_camera(32)
    fb = base.flatten(ctx)
    relit = base.with_lights([sppm.spot_light(T)])
    fv = relit.flatten(ctx)
    p = np.float32([0.8, 0.2, 0.2, 0.0])
    out = C.c_uint32()
    with pytest.raises(T.TraceHipError, match="relit view"):
        ctx.check(L.trhip_scene_add_material(fv._h, 0, T._ffi.fptr(p), 4, C.byref(out)))
    verts, idx, mats = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([1, 2, 3], np.uint32), np.zeros(1, np.uint32)
    with pytest.raises(T.TraceHipError, match="relit view"):
        ctx.check(L.trhip_scene_add_triangles(fv._h, T._ffi.fptr(verts), 3, T._ffi.u32ptr(idx), 1, None, T._ffi.u32ptr(mats), 0, None))
    o2w = np.eye(4, dtype=np.float32)
    with pytest.raises(T.TraceHipError, match="relit view"):
        ctx.check(L.trhip_scene_add_sphere(fv._h, T._ffi.fptr(o2w), T._ffi.fptr(o2w), 0, 0.1, -0.1, 0.1, 360.0, 0, None))
    with pytest.raises(T.TraceHipError, match="relit view"):
        fv.set_bvh(*fv.bvh())
    with pytest.raises(T.TraceHipError, match="shared with a relit view"):
        fb.set_bvh(*fb.bvh())
    h = C.c_void_p()
    ctx.check(L.trhip_scene_new(ctx._h, C.byref(h)))
    v = C.c_void_p()
    try:
        with pytest.raises(T.TraceHipError, match="not committed"):
            ctx.check(L.trhip_scene_relight(h, C.byref(v)))
    finally:
        L.trhip_scene_free(h)
    ctx.check(L.trhip_scene_relight(fb._h, C.byref(v)))
    try:
        with pytest.raises(T.TraceHipError, match="max_node_primitives 4"):
            ctx.check(L.trhip_scene_commit(v, 4))
    finally:
        L.trhip_scene_free(v)
    # the context renders normally afterwards
    check_relit(T, ob, ctx, base, [point(T, (0.3, 0.9, -2.2), 1.5)], cam, "path", 5)
    assert_bits_equal(frame(T, ctx, relit, cam, "path", 5)[0], frame(T, ctx, T.Scene(relit.lights, base.aggregate), cam, "path", 5)[0], "the refused view")
