"""Host side of relit scenes (no GPU): Scene.with_lights keeps the aggregate and takes its bound from the base, and scenes.caustic_moving_lights builds the two lights
of docs/code/caustic_moving.jl:58-89."""

import numpy as np


def test_with_lights_shares_the_aggregate_and_the_bound(T):
    base = T.scenes.cornell_scene()
    sun = T.DirectionalLight(T.translate([0, 0, 0]), T.RGBSpectrum(1.0), np.float32([0.0, 1.0, 0.0]))
    relit = base.with_lights([sun])
    assert relit.aggregate is base.aggregate and relit.lights == [sun] and base.lights != relit.lights
    assert relit._flat is None and base._flat is None  # nothing is flattened before a render asks
    assert np.array_equal(relit.bound, base.bound)
    T.preprocess(sun, relit)
    assert sun.world_radius > 0 and np.array_equal(np.asarray(sun.world_center, np.float32), T.bounding_sphere(base.bound)[0])
    twice = relit.with_lights([])
    assert twice.aggregate is base.aggregate and np.array_equal(twice.bound, base.bound)


def test_caustic_moving_lights(T):
    for shift in (0.0, 0.3, 5.0):
        point, spot = T.scenes.caustic_moving_lights(shift)
        assert isinstance(point, T.PointLight) and isinstance(spot, T.SpotLight)
        assert np.array_equal(point.i.c, np.float32([20, 20, 20]))
        assert np.array_equal(point.light_to_world.m[:3, 3], np.float32([2.5, 10, -100]))
        assert np.array_equal(spot.i.c, np.float32([0.988235, 0.972549, 0.57647]) * np.float32(60))
        assert (spot.total_width, spot.falloff_start) == (30.0, 20.0)
        # light_to_world = translate(4.5, 0, -101) * translate(from) * inv(dir_to_z): the light sits at (4.5, 0.5 + shift, -101) and looks along normalize(to - from)
        assert np.array_equal(spot.light_to_world.m[:3, 3], np.float32([4.5, np.float32(0.5 + shift), -101]))
        axis = spot.light_to_world.m[:3, 2]
        want = np.float32([-5, -(0.5 + shift), 5])
        np.testing.assert_allclose(axis, want / np.linalg.norm(want), rtol=1e-6, atol=1e-6)
