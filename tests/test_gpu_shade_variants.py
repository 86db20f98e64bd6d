"""Every instantiation of the shading kernels against the oracle at full depth, on the scene family of tests/shade_variants.py (its preconditions are asserted on the CPU by
tests/test_shade_variants_scene.py).  The library picks the instantiation from the scene alone — a tangent array, a DirectionalLight, a material-less primitive — and from the
`streaming` option, so each case builds the scene with its switches, asserts them from the scene description, commits it, and hands the oracle the committed tree:
  k_shade_path<STREAM, TAN, DIRL>    classic and streaming x tangents x sun: per-sample radiance, film and ray counts, bit for bit
  k_shade_whitted<0, DIRL>           tangents x sun: the same
  k_shade_sppm<TAN, DIRL, XING>,     tests/test_gpu_sppm.py's run_pair / check_pair with its tolerances; the sun of an SPPM scene is the raw one (zero power, never picked)
  k_shade_photon<TAN, XING>
and the first-hit integrators (feature buffers, ambient occlusion) on the tangent scene against their own references."""
import numpy as np
import pytest

import ao_model as am
import shade_variants as sv
from test_gpu_directional_light import assert_bits_equal
from test_gpu_sppm import check_pair, run_pair

pytestmark = pytest.mark.gpu

_cache = {}


def committed(T, ob, ctx, tangents, sun, crossing=False):
    """(scene, oracle scene on the committed tree), built and committed once per configuration and left alone."""
    key = (tangents, sun, crossing)
    if key not in _cache:
        scene, _ = sv.build(T, tangents, sun, crossing)
        assert sv.switches(T, scene) == key
        flat = scene.flatten(ctx)
        assert "leaf" not in flat.closest_kernel_name(), "the scene must be committed as a hierarchy"
        _cache[key] = (scene, ob.OracleScene.from_scene(scene, bvh=flat.bvh()))
    return _cache[key]


def reference(T, ob, ctx, integrator, depth, tangents, sun):
    key = (integrator, tangents, sun)
    if key not in _cache:
        _, osc = committed(T, ob, ctx, tangents, sun)
        _cache[key] = osc.render(sv.camera(T), integrator, sv.SPP, depth, seed=sv.SEED, want_samples=True)
    return _cache[key]


def render(T, ctx, scene, cls, depth, **options):
    defaults = {"streaming": 0, "stream_budget_min": 2048}
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        integ = cls(sv.camera(T), T.SeededSampler(sv.SPP, seed=sv.SEED), depth)
        film = integ.render(scene, ctx).copy()
        return film, integ.sample_radiance(scene).copy(), integ.stats
    finally:
        for k in options:
            ctx.set_option(k, defaults[k])


def check_against(ref, got, what):
    (ref_film, ref_L, ref_st), (film, L, st) = ref, got
    assert_bits_equal(L, ref_L, f"{what}: per-sample radiance")
    assert_bits_equal(film, ref_film, f"{what}: film")
    assert st.camera_samples == ref_st.camera_samples == sv.SPP * 22 * 26
    assert st.closest_rays == ref_st.closest_rays, f"{what}: closest_rays {st.closest_rays} vs the oracle's {ref_st.closest_rays}"
    assert st.shadow_rays == ref_st.shadow_rays, f"{what}: shadow_rays {st.shadow_rays} vs the oracle's {ref_st.shadow_rays}"


PATH_CASES = [(mode, tangents, sun) for mode in ("classic", "streaming") for tangents in (False, True) for sun in sv.SUNS] + [("streaming_budget_1", True, "preprocessed")]


@pytest.mark.parametrize("mode,tangents,sun", PATH_CASES)
def test_path(T, ob, ctx, mode, tangents, sun):
    scene, _ = committed(T, ob, ctx, tangents, sun)
    assert sv.switches(T, scene) == (tangents, sun, False)
    ref = reference(T, ob, ctx, "path", sv.PATH_DEPTH, tangents, sun)
    assert np.isfinite(ref[1]).all() and (ref[1] > 0).any()
    classic = render(T, ctx, scene, T.PathIntegrator, sv.PATH_DEPTH)
    what = f"path {mode}, tangents={tangents}, sun={sun}"
    if mode == "classic":
        check_against(ref, classic, what)
        return
    got = render(T, ctx, scene, T.PathIntegrator, sv.PATH_DEPTH, streaming=1, **({"stream_budget_min": 1} if mode == "streaming_budget_1" else {}))
    assert got[2].launches_shade > classic[2].launches_shade >= sv.PATH_DEPTH, "the streaming wavefront shades in rounds, more of them than depths: it must not have declined the frame"
    check_against(ref, got, what)
    assert_bits_equal(got[1], classic[1], f"{what}: per-sample radiance, streaming vs classic")
    assert_bits_equal(got[0], classic[0], f"{what}: film, streaming vs classic")
    assert got[2].closest_rays == classic[2].closest_rays and got[2].shadow_rays == classic[2].shadow_rays


@pytest.mark.parametrize("sun", sv.SUNS)
@pytest.mark.parametrize("tangents", [False, True])
def test_whitted(T, ob, ctx, tangents, sun):
    scene, _ = committed(T, ob, ctx, tangents, sun)
    assert sv.switches(T, scene) == (tangents, sun, False)
    ref = reference(T, ob, ctx, "whitted", sv.WHITTED_DEPTH, tangents, sun)
    assert np.isfinite(ref[1]).all() and (ref[1] > 0).any()
    check_against(ref, render(T, ctx, scene, T.WhittedIntegrator, sv.WHITTED_DEPTH), f"whitted, tangents={tangents}, sun={sun}")


# (tangents, sun, crossing): plain, tangents alone, the zero-power sun alone, tangents + sun, crossing + sun + tangents; crossing + tangents is here for its own camera-pass
# instantiation (crossing alone is tests/test_gpu_sppm_materialless.py's)
SPPM_CASES = [(False, "none", False), (True, "none", False), (False, "raw", False), (True, "raw", False), (True, "raw", True), (True, "none", True)]


@pytest.mark.parametrize("tangents,sun,crossing", SPPM_CASES)
def test_sppm(T, ob, ctx, tangents, sun, crossing):
    scene, _ = sv.build(T, tangents, sun, crossing)
    assert sv.switches(T, scene) == (tangents, sun, crossing)
    P = sv.SPPM
    assert T.api.sppm_directional_pick(scene.lights, P["iters"] * P["photons"]) == -1
    integ, xyzw, got, ref = run_pair(T, ob, ctx, scene, sv.camera(T), P["radius"], P["depth"], P["iters"], P["photons"], P["seed"])
    assert "leaf" not in scene.flatten(ctx).closest_kernel_name()
    check_pair(T, xyzw, got, ref, P["iters"])
    assert (got["M"] > 0).mean() > 0.25 and got["info"]["photon_hits"] > 1000, "the photon pass must reach the visible points"
    scene.flatten(ctx).free()
    scene._flat = None


def test_feature_buffers_and_hit_geometry_on_the_tangent_scene(T, ob, ctx):
    """AOVIntegrator's records (t, prim, p, n, ns, material, base colour) against the oracle's closest hits, and the whole rebuilt frame (with ss, which the tangents set)."""
    scene, osc = committed(T, ob, ctx, True, "none")
    cam = sv.camera(T)
    rec = T.AOVIntegrator(cam, T.SeededSampler(sv.SPP, seed=sv.SEED)).samples(scene).reshape(-1)
    rays = ob.generate_rays(cam, T.scenes.camera_sample_grid(cam, sv.SPP, sv.SEED))
    t_ref, prim_ref, geom_ref, _ = osc.trace_closest(rays, want_geom=True)
    hit = prim_ref >= 0
    assert 0.5 < hit.mean() < 1.0
    assert np.array_equal(rec["prim"], prim_ref)
    assert_bits_equal(rec["t"], t_ref, "t")
    for name, cols in (("p", slice(0, 3)), ("n", slice(3, 6)), ("ns", slice(6, 9))):
        assert_bits_equal(rec[name], np.where(hit[:, None], geom_ref[:, cols], np.float32(0.0)), name)
    flat = scene.flatten(ctx)
    assert_bits_equal(flat.hit_geometry(rays)[hit], geom_ref[hit], "hit geometry: p, n, ns, wo, ss")
    _, plain = committed(T, ob, ctx, False, "none")
    assert sv.differs(plain.trace_closest(rays, want_geom=True)[2][hit][:, 12:15], geom_ref[hit][:, 12:15]).mean() > 0.3, "the tangents must set ss"
    ids, cols = T.api.primitive_materials(scene)
    caller = flat.bvh()[3][np.where(hit, prim_ref, 0)]
    assert np.array_equal(rec["material"], np.where(hit, ids[caller], -1))
    assert_bits_equal(rec["albedo"], np.where(hit[:, None], cols[caller], np.float32(0.0)), "albedo")
    assert len(np.unique(rec["material"][hit])) >= 8


def test_ambient_occlusion_on_the_tangent_scene(T, ob, ctx):
    scene, osc = committed(T, ob, ctx, True, "none")
    cam = sv.camera(T)
    ref = am.render(osc, cam, sv.SPP, sv.SEED)
    miss, occluded, opened = am.shares(ref.cls)
    assert min(miss, occluded, opened) >= 0.05, (miss, occluded, opened)
    integ = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(sv.SPP, seed=sv.SEED))
    xyzw = integ.render(scene, ctx)
    assert_bits_equal(integ.sample_radiance(scene), ref.L, "AO per-sample radiance")
    assert np.isfinite(xyzw).all()
    assert integ.stats.shadow_rays == int(ref.hit.sum()) and integ.stats.closest_rays == ref.cls.size
