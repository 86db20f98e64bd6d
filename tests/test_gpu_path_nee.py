"""Next-event estimation of the environment map in path frames on the GPU (trhip_render_path_env_nee; docs/design/28-path-nee.md), bit for bit against the model of
tests/path_nee_model.py: the escape records with their suppressed mark, the per-sample radiance, the film and the frame's shadow-ray count over the parity matrix (four
scenes, two frame sizes, four depths, three mixes, two scales, both settings of HIDE_BACKGROUND, maps of 1, 7 and 64 texels a side under the identity and a turned matrix);
the two identities (scale 0 is trhip_render_path; a scene without a non-specular material is trhip_render_path_env); the frames around a NEE frame; the options the frame
honours and the ones it ignores; the relight's refusal, the device variant, shards, the denoiser and the refusals that need a context.

Shapes: tests/test_gpu_path_env.py's — a 5 x 3 crop under a filter of radius 1/2 at 1 spp (15 samples, fewer than one wave) and 37 x 29 under the default filter at 3 spp
(3627 samples: 56 full waves and a partial one; the all-materials scene's own 26 x 22 x 3).  What the frames contain is asserted from the model, never from the library's
output (tests/test_path_nee_api.py counts the classes of vertices over this matrix)."""
import ctypes as C

import numpy as np
import pytest

import path_env_model as pm
import path_nee_model as nm
import sky_model as sm

pytestmark = pytest.mark.gpu

F = np.float32
SEED = nm.SEED
_envs = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def environment(T, n, turn):
    """The library's Environment over the model's map (tests/path_nee_model.py, env_of), one per process."""
    if (n, turn) not in _envs:
        texels, _, R = nm.env_of(n, turn)
        _envs[n, turn] = T.Environment(texels, R)
    return _envs[n, turn]


def model(T, which, small, depth, mixv, scale, hide, n, turn):
    _, osc = pm.scene_of(T, which, committed=True)
    texels, tab, R = nm.env_of(n, turn)
    return nm.shade(nm.walked(T, which, small, depth, mixv, n, turn, committed=True), texels, tab, R, scale, hide)


def check_frame(T, integ, scene, xyzw, ref, what):
    """Records with their mark, samples, film and shadow-ray count of the frame just rendered against the model's result."""
    beta, depth, dirs = integ.escapes(scene)
    assert_bits_equal(beta, ref.rec[..., 0:3], "beta: " + what)
    assert np.array_equal(depth, ref.rec[..., 3].astype(np.int32)), "escape depth: " + what
    assert_bits_equal(dirs, ref.rec[..., 4:7], "dir: " + what)
    assert np.array_equal(integ.suppressed(scene), ref.rec[..., 7] != 0), "suppressed mark: " + what
    assert_bits_equal(integ.sample_radiance(scene), pm.nan_rule(ref.Lp), "per-sample radiance: " + what)
    assert_bits_equal(xyzw, nm.film(integ.camera, integ.sampler.samples_per_pixel, SEED, integ.sampler.sample_offset, ref.Lp), "film: " + what)
    assert integ.stats.shadow_rays == ref.delta_rays + ref.nee_rays, f"shadow rays {integ.stats.shadow_rays}, the model's {ref.delta_rays} + {ref.nee_rays}: " + what


# ---- the frame against the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nm.matrix(), ids=nm.case_id)
def test_records_samples_film_and_ray_count_equal_the_model(T, ob, ctx, case):
    which, small, depth, mixv, scale, hide, n, turn = case
    scene, _ = pm.scene_of(T, which, committed=True)
    cam, spp, env = pm.camera(T, small, which), 1 if small else 3, environment(T, n, turn)
    ref = model(T, which, small, depth, mixv, scale, hide, n, turn)
    assert small or ref.nee_rays > 500, "the frame casts NEE rays"
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    xyzw = integ.render(scene, environment=env, env_scale=scale, hide_background=hide, env_importance=mixv)
    check_frame(T, integ, scene, xyzw, ref, nm.case_id(case))
    st = integ.stats
    assert st.camera_samples == ref.rec[..., 3].size and st.max_depth_reached == depth and st.launches_shade == depth * st.n_batches


# ---- the two identities --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_scale_zero_is_the_path_frame(T, ob, ctx, which):
    """With scale 0 every NEE contribution and every escape is +0: film and samples are trhip_render_path's bit for bit, though the rays are cast."""
    scene, _ = pm.scene_of(T, which, committed=True)
    cam = pm.camera(T, False, which)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 8)
    film = integ.render(scene).copy()
    L = integ.sample_radiance(scene)
    path_rays = integ.stats.shadow_rays
    got = integ.render(scene, environment=environment(T, 7, True), env_scale=0.0, env_importance=0.5)
    assert_bits_equal(got, film, "film")
    assert_bits_equal(integ.sample_radiance(scene), L, "samples")
    assert integ.stats.shadow_rays > path_rays + 1000, "the NEE rays are cast all the same"
    assert integ.suppressed(scene).sum() > 100
    assert_bits_equal(integ.render(scene), film, "the path frame after it")


def test_a_scene_without_a_non_specular_material_is_the_path_env_frame(T, ob, ctx):
    scene = nm.specular_scene(T)
    cam, env = pm.camera(T), environment(T, 7, True)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 8)
    film = integ.render(scene, environment=env, env_scale=0.5).copy()
    L, rec = integ.sample_radiance(scene), integ.escapes(scene)
    assert (rec[1] >= 2).sum() > 500, "paths do bounce before they leave"
    got = integ.render(scene, environment=env, env_scale=0.5, env_importance=0.25)
    assert_bits_equal(got, film, "film")
    assert_bits_equal(integ.sample_radiance(scene), L, "samples")
    for a, b, what in zip(integ.escapes(scene), rec, ("beta", "depth", "dir")):
        assert_bits_equal(np.asarray(a, F), np.asarray(b, F), what)
    assert not integ.suppressed(scene).any() and integ.stats.shadow_rays == 0


# ---- neighbouring frames -------------------------------------------------------------------------------------------------------------------------------
def test_frames_around_a_nee_frame_keep_their_bits(T, ob, ctx):
    """trhip_render_path, trhip_render_path_env, trhip_render_sky_is and trhip_render_ao on the same context, before and after a NEE frame."""
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam, env = pm.camera(T), environment(T, 7, True)
    path = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 4)
    sky = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, scale=0.5, albedo=True, importance=0.25)
    ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), albedo=True, background=0.25)

    def all_four():
        out = []
        for integ, kw in ((path, {}), (path, dict(environment=env, env_scale=0.5)), (sky, {}), (ao, {})):
            out.append(integ.render(scene, **kw).copy())
            out.append(integ.sample_radiance(scene))
        return out

    before = all_four()
    assert path.render(scene, environment=env, env_scale=0.5, env_importance=True).any()
    names = ("path film", "path samples", "path-env film", "path-env samples", "sky-is film", "sky-is samples", "AO film", "AO samples")
    for got, ref, what in zip(all_four(), before, names):
        assert_bits_equal(got, ref, what + " after a NEE frame")


# ---- options -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["radius-half", "default-filter"])
def test_option_sweep_against_one_reference(T, ob, ctx, small):
    """overlap, pipelines and batch_paths hold and change no bit; streaming and band_tile_rows are ignored; the fused and the sample-major record layout give the same
    records.  The 37 x 29 frame at batch_paths = 1209 (one sample pass of its 39 x 31 sample pixels) runs three batches, on one pipeline or two."""
    which, depth, mixv, n, turn = "cornell", 5, 0.5, 7, True
    scene, _ = pm.scene_of(T, which, committed=True)
    cam, spp, env = pm.camera(T, small, which), 1 if small else 3, environment(T, n, turn)
    ref = model(T, which, small, depth, mixv, 0.5, False, n, turn)
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    defaults = dict(overlap=1, pipelines=1, batch_paths=0, streaming=0, film_fused=1, band_tile_rows=0)
    sweeps = [dict(), dict(overlap=0), dict(pipelines=2), dict(batch_paths=1209), dict(batch_paths=1209, pipelines=2), dict(batch_paths=1209, overlap=0), dict(streaming=1),
              dict(band_tile_rows=1), dict(film_fused=0), dict(film_fused=0, batch_paths=1209, pipelines=2, streaming=1)]
    try:
        for over in sweeps:
            for k, v in {**defaults, **over}.items():
                ctx.set_option(k, v)
            xyzw = integ.render(scene, environment=env, env_scale=0.5, env_importance=mixv)
            check_frame(T, integ, scene, xyzw, ref, f"options {over}")
            if not small:
                assert integ.stats.n_batches == (3 if "batch_paths" in over or "pipelines" in over else 1), over
    finally:
        for k, v in defaults.items():
            ctx.set_option(k, v)


# ---- other behaviour -----------------------------------------------------------------------------------------------------------------------------------
def test_relight_is_refused_after_a_nee_frame(T, ob, ctx):
    scene, _ = pm.scene_of(T, "cornell", committed=True)
    cam, env, L = pm.camera(T, True), environment(T, 7, True), T.lib()
    integ = T.PathIntegrator(cam, T.SeededSampler(1, seed=SEED), 3)
    out = np.zeros((3, 5, 4), F)
    prm = T.api.path_env_params(env, 1.0, False, "test")
    rec = np.zeros(15 * 8, F)
    integ.render(scene, environment=env, env_importance=True)
    assert L.trhip_path_env_relight(ctx._h, env._handle(ctx), C.byref(prm), T._ffi.fptr(out)) == -1 and b"next-event estimation" in L.trhip_last_error(ctx._h)
    assert not out.any()
    assert L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size) == 0, "the records are there"
    with pytest.raises(T.TraceHipError, match="next-event estimation"):
        integ.relight(scene, env)
    integ.render(scene, environment=env)
    assert L.trhip_path_env_relight(ctx._h, env._handle(ctx), C.byref(prm), T._ffi.fptr(out)) == 0, "a path-env frame makes the relight valid again"


def test_determinism_device_variant_and_shards(T, ob, ctx):
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam, env = pm.camera(T), environment(T, 64, False)
    kw = dict(environment=env, env_scale=0.5, env_importance=0.25)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5)
    a = integ.render(scene, **kw).copy()
    La, rec_a, mark_a = integ.sample_radiance(scene), integ.escapes(scene), integ.suppressed(scene)
    assert mark_a.sum() > 100
    assert_bits_equal(integ.render(scene, **kw), a, "film, two calls")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples, two calls")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.render(scene, device_out=d_film.ptr, **kw) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), a, "device variant")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples after the device variant")
    d_film.free()
    shards, recs, marks, films = [], [], [], []
    for spp, off in ((2, 0), (1, 2)):
        s = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED, sample_offset=off), 5)
        films.append(s.render(scene, **kw).copy())
        shards.append(s.sample_radiance(scene))
        recs.append(s.escapes(scene))
        marks.append(s.suppressed(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")
    for k, what in enumerate(("beta", "depth", "dir")):
        assert_bits_equal(np.concatenate([r[k] for r in recs]).astype(F), np.asarray(rec_a[k], F), "records of the shards: " + what)
    assert np.array_equal(np.concatenate(marks), mark_a)
    # films are additive over sample_offset shards up to the order of addition: tests/test_gpu_path_env.py's bound, 48 addends per film pixel on either side
    total = films[0].astype(np.float64) + films[1].astype(np.float64)
    assert np.abs(total - a).max() <= 128 * 2.0 ** -23 * np.abs(a).max()


def test_film_passes_through_the_denoiser(T, ob, ctx):
    import denoise_model as dm
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam = pm.camera(T)
    xyzw = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5).render(scene, environment=environment(T, 7, True), env_scale=0.5, env_importance=True)
    planes = T.AOVIntegrator(cam, T.SeededSampler(3, seed=SEED)).render(scene).planes
    assert_bits_equal(xyzw[..., 3], planes[..., 0, 3], "the NEE film carries the planes' weights")
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    p = d.params
    prm = dm.Params(p.sigma_colour, p.sigma_normal, p.sigma_plane, iterations=p.iterations, demodulate=bool(p.flags & 1), albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)
    assert_bits_equal(out, dm.denoise(xyzw, planes, prm), "the denoiser's model")


def test_refusals_with_a_context(T, ob, ctx):
    import test_gpu_sky as tgs
    scene, _ = pm.scene_of(T, "cornell", committed=True)
    flat, cam, L = scene.flatten(), pm.camera(T, True), T.lib()
    sn, st, out = cam.sensor(), T.Stats(), np.zeros((3, 5, 4), F)
    env = T.Environment(sm.random_map(2))
    bare = T.Environment(sm.random_map(2, seed=9))
    h_env, h_bare = env._sampler_handle(ctx), bare._handle(ctx)  # the second handle has no sampler

    def params(**over):
        p = T._ffi.PathNeeParams()
        assert L.trhip_path_nee_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=1, depth=3, scene_h=flat._h, sensor=sn, outp=T._ffi.fptr(out), context=ctx._h, env_h=h_env):
        return L.trhip_render_path_env_nee(context, scene_h, C.byref(sensor) if sensor is not None else None, spp, depth, SEED, 0, env_h, C.byref(p) if p is not None else None, outp, C.byref(st))

    assert call(params()) == 0 and out.any()
    for over, word in ((dict(scale=-0.5), b"scale"), (dict(flags=2), b"flag"), (dict(mix=0.0), b"mix"), (dict(mix=1.0), b"mix"), (dict(mix=float("nan")), b"mix")):
        assert call(params(**over)) == -1 and word in L.trhip_last_error(ctx._h), over
    # the parameter block before trhip_render_path's refusals, those before the environment's, those before the sampler
    assert call(params(mix=2.0), spp=0, env_h=None) == -1 and b"mix" in L.trhip_last_error(ctx._h)
    assert call(params(), spp=0, env_h=None) == -1 and b"spp" in L.trhip_last_error(ctx._h)
    assert call(params(), depth=0, env_h=h_bare) == -1 and b"max_depth" in L.trhip_last_error(ctx._h)
    assert call(None) == -1 and call(params(), outp=None) == -1 and call(params(), scene_h=None) == -1 and call(params(), sensor=None) == -1 and call(params(), context=None) == -1
    assert call(params(), env_h=None) == -1 and b"null environment" in L.trhip_last_error(ctx._h)
    assert call(params(scale=3.0e38), env_h=h_bare) == -1 and b"+Inf" in L.trhip_last_error(ctx._h), "the scale before the sampler"
    assert call(params(), env_h=h_bare) == -1 and b"no sampler" in L.trhip_last_error(ctx._h)
    assert L.trhip_render_path_env_nee_device(ctx._h, flat._h, C.byref(sn), 1, 3, SEED, 0, h_env, C.byref(params()), None, C.byref(st)) == -1
    holes = tgs.materialless(T)  # material-less primitives: trhip_render_path's refusal, before the environment is looked at
    assert call(params(), scene_h=holes.flatten()._h, env_h=h_bare) == -3 and b"material-less" in L.trhip_last_error(ctx._h)
    other = T.Context(0)  # a second context on the same GPU: its environments are not this context's
    try:
        assert call(params(), env_h=env._handle(other)) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        assert call(params()) == 0
    finally:
        env.close()
        bare.close()
        other.close()
    integ = T.PathIntegrator(cam, T.SeededSampler(1, seed=SEED), 3)
    with pytest.raises(T.TraceHipError, match="sample_map"):
        integ.render(scene, environment=environment(T, 7, True), env_importance=True, sample_map=T.SampleMap(np.ones((3, 5), np.uint32), 1))
    with pytest.raises(T.TraceHipError, match="nothing to sample"):
        integ.render(scene, environment=T.Environment.constant((0, 0, 0)), env_importance=True)  # a black map has no sampler
