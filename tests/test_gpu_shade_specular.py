"""The specular class of k_shade_path (PRIM_SPEC: no light estimate, one sampler case) and the light estimate skipped for BSDFs without a non-specular lobe, against the
oracle bit for bit: film and per-sample radiance of 32 x 32 frames, 4 spp, depth 8, on the scenes of tests/shade_specular_scenes.py (what each one drives is said there).
The ring's wrap-around needs every shading wave to pass the queue at least twice: a 1024 x 1024 frame at 1 spp, whole against bands of one tile row (whose waves see the
queue once and shade their parked entries behind its end), both written by the device entry point.
A smooth glass with allow_multiple_lobes false is two specular lobes; the path integrator never asks for that set (compute_scattering!(si, ray, true)), WhittedIntegrator
does — its frame on S-cornell shows that the new flag bit leaves the kernels alone that read the other set."""
import numpy as np
import pytest

import shade_specular_scenes as ss
from test_gpu_directional_light import assert_bits_equal

pytestmark = pytest.mark.gpu

_cache = {}


def committed(T, ob, ctx, name):
    """(scene, oracle scene on the committed tree): built and committed once per case and left alone."""
    if name not in _cache:
        scene = ss.CASES[name](T)
        _cache[name] = (scene, ob.OracleScene.from_scene(scene, bvh=scene.flatten(ctx).bvh()))
    return _cache[name]


def reference(T, ob, ctx, name, integrator="path"):
    key = (name, integrator)
    if key not in _cache:
        _cache[key] = committed(T, ob, ctx, name)[1].render(ss.camera(T), integrator, ss.SPP, ss.DEPTH, seed=ss.SEED, want_samples=True)
    return _cache[key]


def check(T, ctx, scene, ref, what, cls=None):
    integ = (cls or T.PathIntegrator)(ss.camera(T), T.SeededSampler(ss.SPP, seed=ss.SEED), ss.DEPTH)
    film = integ.render(scene, ctx).copy()
    L = integ.sample_radiance(scene)
    ref_film, ref_L, ref_st = ref
    assert_bits_equal(L, ref_L, f"{what}: per-sample radiance")
    assert_bits_equal(film, ref_film, f"{what}: film")
    assert integ.stats.closest_rays == ref_st.closest_rays and integ.stats.shadow_rays == ref_st.shadow_rays, what
    return integ.stats


@pytest.mark.parametrize("name", list(ss.CASES))
def test_path_against_the_oracle(T, ob, ctx, name):
    scene, _ = committed(T, ob, ctx, name)
    ref = reference(T, ob, ctx, name)
    if name != "lights_none":
        assert np.isfinite(ref[1]).all() and (ref[1] > 0).any(), "the frame must carry light"
    st = check(T, ctx, scene, ref, name)
    if name == "mirror_wall":  # every camera sample hits the mirror: no shadow ray at depth 1, one bounce ray each
        assert st.closest_rays >= 2 * st.camera_samples
    if name == "lights_none":
        assert st.shadow_rays == 0 and not ref[1].any()


@pytest.mark.parametrize("name", ["spec_triangles", "spec_triangles_tangents"])
def test_streaming_wavefront(T, ob, ctx, name):
    scene, _ = committed(T, ob, ctx, name)
    assert "leaf" not in scene.flatten(ctx).closest_kernel_name(), "the scene must be committed as a hierarchy"
    classic = check(T, ctx, scene, reference(T, ob, ctx, name), name)
    ctx.set_option("streaming", 1)
    try:
        st = check(T, ctx, scene, reference(T, ob, ctx, name), name + ", streaming")
    finally:
        ctx.set_option("streaming", 0)
    assert st.launches_shade > classic.launches_shade >= ss.DEPTH, "the streaming wavefront shades in rounds: it must not have declined the frame"


def test_whitted_reads_the_two_lobe_set(T, ob, ctx):
    scene, _ = committed(T, ob, ctx, "s_cornell")
    check(T, ctx, scene, reference(T, ob, ctx, "s_cornell", "whitted"), "whitted on S-cornell", T.WhittedIntegrator)


def test_ring_wraps_around(T, ctx):
    """1024 x 1024, 1 spp, depth 3 on S-cornell: more than 2 x 64 x (shading waves) camera samples, so every wave parks entries in at least two passes and the ring's
    head goes round; the banded frame's waves pass once.  Both films are written on the device (the device entry point); the same bits."""
    scene = T.scenes.cornell_scene()
    cam = T.scenes.cornell_camera(1024)
    h, w = cam.film.size
    whole, banded = T._ffi.DeviceBuffer(h * w * 16).zero(), T._ffi.DeviceBuffer(h * w * 16).zero()
    integ = T.PathIntegrator(cam, T.SeededSampler(1, seed=ss.SEED), 3)
    assert integ.render(scene, ctx, device_out=whole.ptr) is None
    st = integ.stats
    ctx.set_option("band_tile_rows", 1)
    try:
        assert integ.render(scene, ctx, device_out=banded.ptr) is None
    finally:
        ctx.set_option("band_tile_rows", 0)
    assert integ.stats.launches_shade > st.launches_shade, "the second frame must have been rendered in bands"
    a, b = whole.to_host(np.uint32, (h, w, 4)), banded.to_host(np.uint32, (h, w, 4))
    whole.free()
    banded.free()
    assert np.isfinite(a.view(np.float32)).all() and (a.view(np.float32)[..., 3] > 0).any() and (a.view(np.float32)[..., :3] > 0).any()
    assert np.array_equal(a, b), f"{int((a != b).sum())} film values differ between the whole and the banded frame"
