"""DirectionalLight on the host side (no GPU): the mirror's fields, Scene.bound, bounding_sphere, preprocess and SPPM's refusal rule,
against values built from the oracle's pinned pieces (orc_scene_world_bound, orc_radical_inverse, orc_sample_discrete)."""
import numpy as np
import pytest

import directional_model as dm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_direction_is_the_normalised_world_vector(T):
    for l2w, d in ((T.translate([3.0, -2.0, 7.0]), [-0.35, 1.0, 0.45]), (T.scale(2.0, 0.5, 3.0), [0.1, -1.0, 0.2]),
                   (T.look_at([1, 2, 3], [0, 0, 0], [0, 1, 0]), [0.0, 0.0, 1.0])):
        light = T.DirectionalLight(l2w, T.RGBSpectrum(2.0), np.float32(d))
        m, v = l2w.m, np.float32(d)
        w = np.array([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)], np.float32)  # transformations.jl:139: no translation
        n = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        assert np.array_equal(bits(light.direction), bits((f32(1.0) / n) * w))
        assert light.world_radius == 0 and not np.any(light.world_center)  # directional.jl:30


def _scenes(T):
    yield "triangles", dm.floor_scene(T, preprocessed=False, special=False)
    core = T.ShapeCore(T.translate([0.25, -0.5, 1.5]) * T.scale(1.0, 2.0, 0.5), False)
    spheres = [T.GeometricPrimitive(T.Sphere(core, 0.7, -0.2, 0.5, 270.0), None),
               T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.look_at([1, 2, 3], [0, 0, 0], [0, 1, 0]), True), 0.3, 0.9, -2.0, 180.0), None)]
    yield "partial spheres", T.Scene([], T.BVHAccel(spheres, 1))
    inner = T.BVHAccel(list(dm.floor_scene(T, preprocessed=False).aggregate.primitives[:4]), 2)
    empty = T.BVHAccel([], 1)
    yield "nested", T.Scene([], T.BVHAccel([inner, empty, spheres[0]], 1))
    yield "empty", T.Scene([], T.BVHAccel([], 1))


def test_scene_bound_equals_the_reference_world_bound(T, ob):
    for name, scene in _scenes(T):
        b = scene.bound
        if not T.api.splice_nested(scene.aggregate.primitives):
            assert np.array_equal(bits(b), bits([np.inf] * 3 + [-np.inf] * 3)), name  # Bounds3()
            continue
        osc = ob.OracleScene.from_scene(T.Scene([], scene.aggregate))
        assert np.array_equal(bits(b), bits(osc.world_bound())), name


def test_bounding_sphere_and_preprocess(T):
    b = np.float32([-1.0, 0.0, -3.0, 1.0, 1.5, -2.0])
    c, r = T.bounding_sphere(b)
    want_c = (b[:3] + b[3:]) / f32(2.0)
    dv = want_c - b[3:]
    assert np.array_equal(bits(c), bits(want_c)) and bits(r) == bits(np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]))
    c, r = T.bounding_sphere([np.inf] * 3 + [-np.inf] * 3)  # an empty box: the center is not inside, radius 0f0
    assert r == 0
    scene = dm.floor_scene(T, preprocessed=False)
    light = scene.lights[0]
    assert light.world_radius == 0
    scene._flat = "stale"
    T.preprocess(light, scene)
    c, r = T.bounding_sphere(scene.bound)
    assert bits(light.world_radius) == bits(r) and r > 0 and np.array_equal(bits(light.world_center), bits(c))
    assert scene._flat is None  # the flattened scene held the old fields


@pytest.mark.parametrize("index", [0, 1, (1 << 25) - 2, (1 << 25) - 1, (1 << 26) - 1, 3 * (1 << 25) - 1, (1 << 24) - 1, (1 << 25) + (1 << 24) - 1,
                                   ((1 << 24) - 1) | (((1 << 54) - 1) ^ ((1 << 25) - 1)), ((1 << 24) - 1) | (((1 << 53) - 1) ^ ((1 << 25) - 1))])
def test_radical_inverse_is_one_matches_the_oracle(T, ob, index):
    u = ob.lib().orc_radical_inverse(0, index)
    assert T.api.radical_inverse_is_one(index, index + 1) == (u == 1.0)


def test_three_photons_of_c4_reach_the_last_light():
    P, it = 1046529, 100
    n = sum(1 for k in range(1, 4) if k * (1 << 25) - 1 < P * it)
    assert n == 3


def _picked_by_oracle(ob, func, u):
    out = np.empty(3, np.float32)
    fn = np.ascontiguousarray(func, np.float32)
    ob.lib().orc_sample_discrete(ob.fp(fn), fn.size, f32(u), ob.fp(out))
    return int(out[0]) - 1


def test_sppm_refusal_rule(T, ob):
    pick = T.api.sppm_directional_pick
    sun = dm.sun(T)
    point = T.PointLight(T.translate([0, 1, 0]), T.RGBSpectrum(2.0))
    dark = T.PointLight(T.translate([0, 1, 0]), T.RGBSpectrum(0.0))
    # (a) a preprocessed light has power (I·π)·r² > 0
    lit = dm.floor_scene(T, preprocessed=True)
    assert pick(lit.lights, 1000) == 0
    assert pick([point] + lit.lights, 1000) == 1
    # (b) every light's power is 0: the CDF is uniform-ish (sampling.jl:18-21) and gives the first light [0, 2/n)
    assert pick([sun], 1) == 0
    assert pick([sun, dark], 1) == 0
    # (c) a zero-power light placed last is picked only for u == 1f0, i.e. a Halton index = 2^25 - 1 (mod 2^25) in the range
    assert pick([point, sun], (1 << 25) - 1) == -1
    assert pick([point, sun], 1 << 25) == 1
    assert pick([point, sun], 1000, first_index=3 * (1 << 25) - 10) == 1
    assert pick([point, sun], 1000, first_index=3 * (1 << 25)) == -1
    assert pick([dark, sun], 1 << 25) == 1 and pick([dark, sun], 1000) == -1
    # a zero-power light first beside a point light has an interval of zero width: never picked
    assert pick([sun, point], 1 << 30) == -1
    # the intervals the rule reads are sample_discrete's (the oracle's mirror of sampling.jl:32-41)
    func = np.array([T.api.light_power_y(l) for l in (sun, point)], np.float32)
    assert all(_picked_by_oracle(ob, func, u) == 1 for u in (0.0, 0.3, 0.999, 1.0))
    func = np.array([T.api.light_power_y(l) for l in (point, sun)], np.float32)
    assert _picked_by_oracle(ob, func, 1.0) == 1 and _picked_by_oracle(ob, func, np.nextafter(f32(1.0), f32(0.0))) == 0
    u_one = ob.lib().orc_radical_inverse(0, (1 << 25) - 1)
    assert u_one == 1.0 and _picked_by_oracle(ob, func, u_one) == 1
    func = np.zeros(3, np.float32)
    assert [_picked_by_oracle(ob, func, u) for u in (0.0, 0.6, 0.7, 1.0)] == [0, 0, 1, 2]


def test_light_power_matches_the_reference_formula(T):
    sun = dm.sun(T)
    assert T.api.light_power_y(sun) == 0
    sun.world_radius = f32(1.75)
    I = np.asarray(sun.i.c, np.float32)
    power = (I * f32(np.pi)) * (f32(1.75) * f32(1.75))  # directional.jl:54-56
    want = f32(f32(f32(0.212671) * power[0]) + f32(f32(0.715160) * power[1])) + f32(f32(0.072169) * power[2])
    assert bits(T.api.light_power_y(sun)) == bits(want)


@pytest.mark.parametrize("integrator", ["whitted", "path"])
@pytest.mark.parametrize("material", ["matte", "plastic"])
def test_the_composite_model_is_the_oracle_render_on_point_lights(T, ob, integrator, material):
    """The model of tests/directional_model.py, run on the scene's point light alone, against the oracle's own render at depth 1: bit for bit
    wherever the model says its BSDF frame is the render's, within 8 ulp elsewhere."""
    scene = dm.floor_scene(T, material, "point_first", preprocessed=False)
    plain = T.Scene([scene.lights[0]], scene.aggregate)
    bvh = ob.OracleScene.from_scene(plain).get_bvh()
    cam = T.scenes.shadows_camera(64)
    _, ref, _ = ob.OracleScene.from_scene(plain, bvh=bvh).render(cam, integrator, 4, 1, seed=11, want_samples=True)
    want, exact = dm.direct_terms(T, ob, plain, cam, 4, 11, integrator, bvh=bvh)
    ref = ref.reshape(want.shape)
    assert exact.mean() > 0.9 and (want > 0).any()
    assert np.array_equal(bits(ref)[exact], bits(want)[exact])
    assert np.abs(bits(ref).view(np.int32).astype(np.int64) - bits(want).view(np.int32).astype(np.int64)).max() <= 8
