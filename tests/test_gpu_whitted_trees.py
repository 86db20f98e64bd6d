"""WhittedIntegrator on WIDE ray trees (tests/whitted_trees.py): levels that hold many times the rays of the camera level, interior nodes whose two children both have
two children, one to three lights on every node.  Every frame must equal the oracle's recursion bit for bit, per sample and in the film, with the oracle's ray counts —
also the frames whose trees do not fit the level queues in one go (render_whitted_impl cuts those into smaller batches of camera rays), however the frame was cut, and
whatever ran on the context before.

Each test asserts from the oracle's ray counts that its tree is as wide as it is meant to be: a scene that stopped branching cannot pass silently."""
import numpy as np
import pytest

import whitted_trees as wt
from test_gpu_parity import assert_bits_equal, scene_pair

pytestmark = pytest.mark.gpu
_cache = {}


def pair(T, ob, name, lights="point"):
    """(scene, the oracle's frames of it), built once per module run."""
    if (name, lights) not in _cache:
        scene = wt.make_scene(T, name, lights)
        _, osc = scene_pair(T, ob, scene)
        _cache[name, lights] = (scene, wt.OracleFrames(T, osc))
    return _cache[name, lights]


def widths(T, ob, name, res, spp, depth, levels=None):
    """Rays per camera ray at the levels of the tree; the lights do not change the tree, so the point-light frames serve every light set."""
    return pair(T, ob, name)[1].rays_per_camera_ray(res, spp, depth, levels)


def gpu_frame(T, scene, res, spp, depth, sample_offset=0, device=False):
    cam = T.scenes.cornell_camera(res)
    integ = T.WhittedIntegrator(cam, T.SeededSampler(spp, seed=wt.SEED, sample_offset=sample_offset), depth)
    if device:
        h, w = cam.film.size
        d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
        try:
            assert integ.render(scene, device_out=d_film.ptr) is None
            xyzw = d_film.to_host(np.float32, (h, w, 4))
        finally:
            d_film.free()
    else:
        xyzw = integ.render(scene).copy()
    return xyzw, integ.sample_radiance(scene), integ.stats


def assert_equals_oracle(T, ob, name, lights, res, spp, depth, sample_offset=0):
    scene, frames = pair(T, ob, name, lights)
    ref_xyzw, ref_L, st = frames.frame(res, spp, depth, sample_offset=sample_offset)
    xyzw, L, stats = gpu_frame(T, scene, res, spp, depth, sample_offset)
    what = f"{name} / {lights} {res}x{res} {spp} spp depth {depth}"
    if lights == "point_front" and depth >= 2:  # the one light set that sends radiance up the tree (whitted_trees.LIGHT_SETS): nearly every sample is a sum of lit leaves
        assert (ref_L.max(axis=-1) > 0).mean() > 0.9, what
        if name == "window":  # … and the ground leaves the window's tree as it was: the preconditions counted on the point-light scene hold here
            assert st.closest_rays == pair(T, ob, name)[1].frame(res, spp, depth, sample_offset=sample_offset)[2].closest_rays, what
    assert_bits_equal(L, ref_L, f"{what}: per-sample radiance")
    assert_bits_equal(xyzw, ref_xyzw, f"{what}: film")
    assert (stats.closest_rays, stats.shadow_rays) == (st.closest_rays, st.shadow_rays), f"{what}: ray counts"
    assert stats.n_batches >= 1
    return xyzw, L, stats


# ---- 1. wide trees on the smallest film -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", wt.LIGHT_SETS)
@pytest.mark.parametrize("depth", range(1, 8))
def test_window_every_depth_every_light_set(T, ob, ctx, depth, lights):
    """Four glass interfaces: from level 4 on, interior nodes have two children that both have two children; one or two lights add to every node in light order, the
    directional light runs k_shade_whitted<0, true>, and under "point_front" every level has lit leaves."""
    w = widths(T, ob, "window", 32, 2, 7)
    assert w[7] >= 10, w  # measured 14.5
    assert_equals_oracle(T, ob, "window", lights, 32, 2, depth)


def test_nested_spheres(T, ob, ctx):
    """Three concentric glass spheres: rays bounce between the shells, the tree is ragged (leaves at every level)."""
    w = widths(T, ob, "nested", 32, 2, 7)
    assert w[2] < 1 and w[7] >= 2.4, w  # camera rays that miss the spheres are leaves at level 1; measured 0.66 and 2.66
    assert_equals_oracle(T, ob, "nested", "point", 32, 2, 7)


def test_pane_in_front_of_a_sphere_two_lights(T, ob, ctx):
    w = widths(T, ob, "pane_sphere", 48, 2, 6)
    assert w[6] >= 3, w  # measured 3.3
    assert_equals_oracle(T, ob, "pane_sphere", "point_spot", 48, 2, 6)


# ---- 2. trees wider than the queues of a whole sample pass --------------------------------------------------------------------------
TOO_WIDE = [
    # scene, lights, res, depth, the level that outgrows its queue and the rays per camera ray it must hold at least (measured: 5.5, 3.8, 23.0, 3.9)
    ("window", "point", 96, 5, 5, 5.0),
    ("window", "point", 128, 4, 4, 3.6),
    ("window", "point", 32, 8, 8, 22.0),
    ("pane_sphere", "point_spot", 128, 7, 7, 3.6),
    ("window", "point_front", 96, 5, 5, 5.0),  # the first frame again, with radiance in its tree
]


def assert_too_wide_for_one_pass(T, ob, name, res, depth, level, at_least):
    w = widths(T, ob, name, res, 1, depth, levels=(level,))[level]
    slots = wt.queue_slots_per_camera_ray((res + 2) ** 2)
    assert w >= at_least and w > slots, f"level {level} holds {w:.2f} rays per camera ray, its queue {slots:.2f} slots"


@pytest.mark.parametrize("name,lights,res,depth,level,at_least", TOO_WIDE)
def test_tree_wider_than_a_sample_pass_of_queues(T, ob, ctx, name, lights, res, depth, level, at_least):
    """A level that cannot fit the queues sized for one sample pass (a pigeonhole argument on the oracle's count) renders all the same, and a ray traced in an attempt that
    was abandoned counts once."""
    assert_too_wide_for_one_pass(T, ob, name, res, depth, level, at_least)
    assert_equals_oracle(T, ob, name, lights, res, 1, depth)


# ---- 3. nothing depends on how the frame was cut ------------------------------------------------------------------------------------
def test_window_cut_four_ways(T, ob, ctx):
    res, spp, depth = 64, 3, 6
    scene, frames = pair(T, ob, "window", "point_front")
    ref_xyzw, ref_L, st = frames.frame(res, spp, depth)
    assert widths(T, ob, "window", res, spp, depth, levels=(6,))[6] >= 8  # measured 9.0
    assert st.closest_rays == pair(T, ob, "window")[1].frame(res, spp, depth)[2].closest_rays and (ref_L.max(axis=-1) > 0).mean() > 0.9  # the same tree, lit
    npix = wt.sample_pixels(T.scenes.cornell_camera(res))
    got = {}
    try:
        for how, batch_paths in (("free memory", 0), ("one sample pass", npix), ("three passes", 3 * npix)):
            ctx.set_option("batch_paths", batch_paths)
            got[how] = gpu_frame(T, scene, res, spp, depth)
    finally:
        ctx.set_option("batch_paths", 0)
    got["device entry point"] = gpu_frame(T, scene, res, spp, depth, device=True)
    for how, (xyzw, L, stats) in got.items():
        assert_bits_equal(L, ref_L, f"{how}: per-sample radiance")
        assert_bits_equal(xyzw, ref_xyzw, f"{how}: film")
        assert (stats.closest_rays, stats.shadow_rays) == (st.closest_rays, st.shadow_rays), how
        assert stats.n_batches >= 1
    again = gpu_frame(T, scene, res, spp, depth)
    assert again[2].n_batches == got["free memory"][2].n_batches, "n_batches of two identical calls"


def test_window_sample_offset(T, ob, ctx):
    assert_equals_oracle(T, ob, "window", "point_front", 64, 2, 6, sample_offset=2)


@pytest.mark.parametrize("option,value,default", [("traversal", 1, 3), ("hybrid", 0, 1)])
def test_window_other_walks_same_bits(T, ob, ctx, option, value, default):
    scene, _ = pair(T, ob, "window", "point_front")
    a = gpu_frame(T, scene, 64, 3, 6)
    ctx.set_option(option, value)
    try:
        b = gpu_frame(T, scene, 64, 3, 6)
    finally:
        ctx.set_option(option, default)
    assert_bits_equal(b[1], a[1], f"{option} = {value}: per-sample radiance")
    assert_bits_equal(b[0], a[0], f"{option} = {value}: film")
    assert (b[2].closest_rays, b[2].shadow_rays) == (a[2].closest_rays, a[2].shadow_rays)


# ---- 4. nothing carries over --------------------------------------------------------------------------------------------------------
def test_nothing_carries_over(T, ob, ctx):
    """A frame that had to be cut, then test_whitted_shadows_bit_exact's 48² / depth 5 frame, then a PathIntegrator frame of the same scene, on one context: each equals
    its oracle; and the first frame once more has the bits and the stats of its first run."""
    name, lights, res, depth, level, at_least = TOO_WIDE[-1]
    assert_too_wide_for_one_pass(T, ob, name, res, depth, level, at_least)
    xyzw1, L1, stats1 = assert_equals_oracle(T, ob, name, lights, res, 1, depth)
    shadows = T.scenes.shadows_scene()
    _, osc = scene_pair(T, ob, shadows)
    cam = T.scenes.shadows_camera(48)
    for cls, which, spp, d, seed in ((T.WhittedIntegrator, "whitted", 2, 5, 0x5EED0001), (T.PathIntegrator, "path", 2, 5, 7)):
        integ = cls(cam, T.SeededSampler(spp, seed=seed), d)
        xyzw = integ.render(shadows)
        ref_xyzw, ref_L, st = osc.render(cam, which, spp, d, seed=seed, want_samples=True)
        assert ref_L.max() > 0
        assert_bits_equal(integ.sample_radiance(shadows), ref_L, f"{which} on the shadows scene: per-sample radiance")
        assert_bits_equal(xyzw, ref_xyzw, f"{which} on the shadows scene: film")
        assert (integ.stats.closest_rays, integ.stats.shadow_rays) == (st.closest_rays, st.shadow_rays)
    xyzw2, L2, stats2 = assert_equals_oracle(T, ob, name, lights, res, 1, depth)
    assert_bits_equal(L2, L1, "second run: per-sample radiance")
    assert_bits_equal(xyzw2, xyzw1, "second run: film")
    assert stats2.n_batches == stats1.n_batches
