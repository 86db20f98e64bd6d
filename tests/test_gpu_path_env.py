"""The environment term of path frames on the GPU (trhip_render_path_env, trhip_last_escapes, trhip_path_env_relight; docs/design/26-path-env.md), bit for bit against the
model of tests/path_env_model.py: the escape records, the per-sample radiance and the film on four scenes, two frame sizes, four depths, two scales and both settings of
HIDE_BACKGROUND; the anchors through existing code (scale 0 is trhip_render_path; the frames around a path-env frame keep their bits); the options the frame honours and the
ones it ignores, in both record layouts; the relight against a fresh frame; the device variants, shards, determinism, the denoiser and the refusals that need a context.

Shapes: a 5 x 3 crop under a filter of radius 1/2 at 1 spp (15 samples, fewer than one wave) and 37 x 29 under the default Lanczos filter at 3 spp (39 x 31 x 3 = 3627
samples: 56 full waves and a partial one; the all-materials scene's own 26 x 22 x 3).  What the frames contain is asserted from the model, never from the library's output."""
import ctypes as C

import numpy as np
import pytest

import path_env_model as pm
import sky_model as sm

pytestmark = pytest.mark.gpu

F = np.float32
SEED = pm.SEED


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


_env = {}


def sky_map(T, second=False):
    """A 7 x 7 map of unequal texels under a turned matrix; `second`: another map (5 x 5, another seed) under another turn, for the relight."""
    if second not in _env:
        _env[second] = T.Environment(sm.random_map(5, seed=23), sm.rotation((0.7, 0.2, -0.4), 2.3)) if second else T.Environment(sm.random_map(7), sm.rotation())
    return _env[second]


def model(T, which, small, depth, env, scale, hide):
    scene, osc = pm.scene_of(T, which, committed=True)
    cam, spp = pm.camera(T, small, which), 1 if small else 3
    return pm.render(osc, cam, spp, depth, SEED, 0, env.texels, env.world_to_env, scale, hide, walked=pm.walked(T, which, small, depth, committed=True))


def check_frame(T, integ, scene, xyzw, ref, what):
    """Records, samples and film of the frame just rendered against the model's result."""
    beta, depth, dirs = integ.escapes(scene)
    assert_bits_equal(beta, ref.beta, "beta: " + what)
    assert np.array_equal(depth, ref.depth), "escape depth: " + what
    assert_bits_equal(dirs, ref.dir, "dir: " + what)
    assert_bits_equal(integ.sample_radiance(scene), pm.nan_rule(ref.Lp), "per-sample radiance: " + what)
    spp = integ.sampler.samples_per_pixel
    assert_bits_equal(xyzw, pm.film(integ.camera, spp, SEED, integ.sampler.sample_offset, ref.Lp), "film: " + what)


# ---- the frame against the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["5x3-1spp", "37x29-3spp"])
@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_records_samples_and_film_equal_the_model(T, ob, ctx, which, small):
    scene, _ = pm.scene_of(T, which, committed=True)
    cam, spp, env = pm.camera(T, small, which), 1 if small else 3, sky_map(T)
    assert tuple(cam.film.size) == ((3, 5) if small else (20, 24) if which == "materials" else (29, 37))
    for depth in pm.DEPTHS:
        integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
        for scale in (0.5, 0.0):
            for hide in (False, True):
                what = f"{which}, depth {depth}, scale {scale}, hide_background {hide}"
                ref = model(T, which, small, depth, env, scale, hide)
                assert set(np.unique(ref.depth)) == set(range(0, depth + 1)) or small, "the model's frame holds escapes of every depth, and paths without one"
                assert small or depth == 1 or hide or scale == 0.0 or (bits(ref.Lp) != bits(ref.L)).any(axis=-1).sum() > 100, "the escapes read the map"
                xyzw = integ.render(scene, environment=env, env_scale=scale, hide_background=hide)
                check_frame(T, integ, scene, xyzw, ref, what)
                st = integ.stats
                assert st.camera_samples == ref.depth.size and st.max_depth_reached == depth and st.launches_shade == depth * st.n_batches, "statistics are trhip_render_path's"


@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_scale_zero_is_the_path_frame(T, ob, ctx, which):
    """The anchor through existing code: with scale 0 film and samples are trhip_render_path's bit for bit."""
    scene, _ = pm.scene_of(T, which, committed=True)
    cam = pm.camera(T, False, which)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 8)
    film = integ.render(scene).copy()
    L = integ.sample_radiance(scene)
    assert film[..., :3].any() or which == "unlit"
    got = integ.render(scene, environment=sky_map(T), env_scale=0.0)
    assert_bits_equal(got, film, "film")
    assert_bits_equal(integ.sample_radiance(scene), L, "samples")
    _, depth, _ = integ.escapes(scene)
    assert (depth > 0).sum() > 100, "the records are written all the same"
    assert_bits_equal(integ.render(scene), film, "the path frame after it")


def test_frames_around_a_path_env_frame_keep_their_bits(T, ob, ctx):
    """trhip_render_path, trhip_render_sky and trhip_render_ao on the same context, before and after a path-env frame."""
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam, env = pm.camera(T), sky_map(T)
    path = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 4)
    sky = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, scale=0.5, albedo=True)
    ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), albedo=True, background=0.25)

    def all_three():
        out = []
        for integ in (path, sky, ao):
            out.append(integ.render(scene).copy())
            out.append(integ.sample_radiance(scene))
        return out

    before = all_three()
    assert path.render(scene, environment=env, env_scale=0.5).any()
    for got, ref, what in zip(all_three(), before, ("path film", "path samples", "sky film", "sky samples", "AO film", "AO samples")):
        assert_bits_equal(got, ref, what + " after a path-env frame")


# ---- options -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["radius-half", "default-filter"])
def test_option_sweep_against_one_reference(T, ob, ctx, small):
    """overlap, pipelines and batch_paths hold and change no bit; streaming and band_tile_rows are ignored; the fused and the sample-major record layout give the same
    records.  The 37 x 29 frame at batch_paths = 1209 (one sample pass of its 39 x 31 sample pixels) runs three batches, on one pipeline or two; the crop's 15 samples are one batch anyway."""
    which, depth = "cornell", 5
    scene, _ = pm.scene_of(T, which, committed=True)
    cam, spp, env = pm.camera(T, small, which), 1 if small else 3, sky_map(T)
    ref = model(T, which, small, depth, env, 0.5, False)
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    defaults = dict(overlap=1, pipelines=1, batch_paths=0, streaming=0, film_fused=1, band_tile_rows=0)
    sweeps = [dict(), dict(overlap=0), dict(pipelines=2), dict(batch_paths=1209), dict(batch_paths=1209, pipelines=2), dict(batch_paths=1209, overlap=0), dict(streaming=1),
              dict(band_tile_rows=1), dict(film_fused=0), dict(film_fused=0, batch_paths=1209, pipelines=2, streaming=1)]
    try:
        for over in sweeps:
            for k, v in {**defaults, **over}.items():
                ctx.set_option(k, v)
            xyzw = integ.render(scene, environment=env, env_scale=0.5)
            check_frame(T, integ, scene, xyzw, ref, f"options {over}")
            if not small:
                # (two pipelines cut the frame into batches of floor(3 / 2) = 1 sample pass as well: at least as many batches as pipelines)
                assert integ.stats.n_batches == (3 if "batch_paths" in over or "pipelines" in over else 1), over
    finally:
        for k, v in defaults.items():
            ctx.set_option(k, v)


# ---- relight -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["5x3-1spp", "37x29-3spp"])
def test_relight_equals_a_fresh_frame(T, ob, ctx, small):
    which, depth = "materials", 8
    scene, _ = pm.scene_of(T, which, committed=True)
    cam, spp, env1, env2 = pm.camera(T, small, which), 1 if small else 3, sky_map(T), sky_map(T, second=True)
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    fresh2 = integ.render(scene, environment=env2, env_scale=1.5, hide_background=True).copy()
    L2 = integ.sample_radiance(scene)
    first = integ.render(scene, environment=env1, env_scale=0.5).copy()
    L1 = integ.sample_radiance(scene)
    assert (bits(L1) != bits(L2)).any(axis=-1).sum() > (5 if small else 100)
    assert_bits_equal(integ.relight(scene, env2, env_scale=1.5, hide_background=True), fresh2, "relit film")
    assert_bits_equal(integ.sample_radiance(scene), L2, "relit samples")
    check_frame(T, integ, scene, fresh2, model(T, which, small, depth, env2, 1.5, True), "the relit frame against the model")
    assert_bits_equal(integ.relight(scene, env1, env_scale=0.5), first, "relit back: film")
    assert_bits_equal(integ.sample_radiance(scene), L1, "relit back: samples")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.relight(scene, env2, env_scale=1.5, hide_background=True, device_out=d_film.ptr) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), fresh2, "device variant of the relight")
    d_film.free()


def test_relight_and_records_are_refused_after_another_frame(T, ob, ctx):
    scene, _ = pm.scene_of(T, "cornell", committed=True)
    cam, env, L = pm.camera(T, True), sky_map(T), T.lib()
    integ = T.PathIntegrator(cam, T.SeededSampler(1, seed=SEED), 3)
    out = np.zeros((3, 5, 4), F)
    prm = T.api.path_env_params(env, 1.0, False, "test")
    rec = np.zeros(15 * 8, F)

    def relight():
        return L.trhip_path_env_relight(ctx._h, env._handle(ctx), C.byref(prm), T._ffi.fptr(out))

    integ.render(scene, environment=env)
    assert relight() == 0 and L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size) == 0
    assert L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size - 8) == -1 and b"expected 120 floats" in L.trhip_last_error(ctx._h)
    integ.render(scene)  # trhip_render_path in between
    assert relight() == -1 and b"not a path-env frame" in L.trhip_last_error(ctx._h)
    assert L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size) == -1 and b"not a path-env frame" in L.trhip_last_error(ctx._h)
    with pytest.raises(T.TraceHipError):
        integ.relight(scene, env)
    xyzw = integ.render(scene, environment=env)
    planes = T.AOVIntegrator(cam, T.SeededSampler(1, seed=SEED)).render(scene).planes  # another render in between
    assert relight() == -1
    integ.render(scene, environment=env)
    T.Denoiser().denoise(xyzw, planes, ctx)  # an image pass in between
    assert relight() == -1
    integ.render(scene, environment=env)
    film = np.empty_like(out)
    ctx.check(L.trhip_film_accumulate(ctx._h, C.byref(cam.sensor()), 1, SEED, 0, T._ffi.fptr(np.zeros((1, 3, 5, 3), F)), T._ffi.fptr(film)))  # a film call in between
    assert relight() == -1
    integ.render(scene, environment=env)
    assert relight() == 0, "a fresh frame makes it valid again"


# ---- other frame properties ----------------------------------------------------------------------------------------------------------------------------------
def test_determinism_device_variant_and_shards(T, ob, ctx):
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam, env = pm.camera(T), sky_map(T)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5)
    a = integ.render(scene, environment=env, env_scale=0.5).copy()
    La, rec_a = integ.sample_radiance(scene), integ.escapes(scene)
    assert_bits_equal(integ.render(scene, environment=env, env_scale=0.5), a, "film, two calls")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples, two calls")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.render(scene, environment=env, env_scale=0.5, device_out=d_film.ptr) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), a, "device variant")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples after the device variant")
    d_film.free()
    shards, recs, films = [], [], []
    for spp, off in ((2, 0), (1, 2)):
        s = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED, sample_offset=off), 5)
        films.append(s.render(scene, environment=env, env_scale=0.5).copy())
        shards.append(s.sample_radiance(scene))
        recs.append(s.escapes(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")
    for k, what in enumerate(("beta", "depth", "dir")):
        assert_bits_equal(np.concatenate([r[k] for r in recs]).astype(F), np.asarray(rec_a[k], F), "records of the shards: " + what)
    # films are additive over sample_offset shards: the same samples splat with the same weights, in another order of addition.  A film pixel sums at most 4 x 4 sample
    # pixels x 3 samples = 48 addends (filter radius 1), each addition rounds by at most 2^-24 of a partial sum, and the partial sums stay below twice the largest film value
    # (Lanczos' negative lobe is a small share of its mass): 48 * 2^-24 * 2 * max|film| on either side, 128 * 2^-23 * max|film| with a margin for the two orders together.
    total = films[0].astype(np.float64) + films[1].astype(np.float64)
    assert np.abs(total - a).max() <= 128 * 2.0 ** -23 * np.abs(a).max()


def test_film_passes_through_the_denoiser(T, ob, ctx):
    import denoise_model as dm
    scene, _ = pm.scene_of(T, "mesh", committed=True)
    cam = pm.camera(T)
    xyzw = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5).render(scene, environment=sky_map(T), env_scale=0.5)
    planes = T.AOVIntegrator(cam, T.SeededSampler(3, seed=SEED)).render(scene).planes
    assert_bits_equal(xyzw[..., 3], planes[..., 0, 3], "the path-env film carries the planes' weights")
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    p = d.params
    prm = dm.Params(p.sigma_colour, p.sigma_normal, p.sigma_plane, iterations=p.iterations, demodulate=bool(p.flags & 1), albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)
    surface = dm.surface_mask(xyzw, planes, prm)
    assert surface.sum() > 50 and (~surface).sum() > 20
    assert_bits_equal(out[~surface], xyzw[~surface], "non-surface pixels (the sky among them) pass through")
    assert_bits_equal(out, dm.denoise(xyzw, planes, prm), "the denoiser's model")


def test_refusals_with_a_context(T, ob, ctx):
    import test_gpu_sky as tgs
    scene, _ = pm.scene_of(T, "cornell", committed=True)
    flat, cam, L = scene.flatten(), pm.camera(T, True), T.lib()
    sn, st, out = cam.sensor(), T.Stats(), np.zeros((3, 5, 4), F)
    env = T.Environment(sm.random_map(2))
    h_env = env._handle(ctx)

    def params(**over):
        p = T._ffi.PathEnvParams()
        assert L.trhip_path_env_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=1, depth=3, scene_h=flat._h, sensor=sn, outp=T._ffi.fptr(out), context=ctx._h, env_h=h_env):
        return L.trhip_render_path_env(context, scene_h, C.byref(sensor) if sensor is not None else None, spp, depth, SEED, 0, env_h, C.byref(p) if p is not None else None, outp, C.byref(st))

    assert call(params()) == 0 and out.any()
    for over, word in ((dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"), (dict(flags=2), b"flag")):
        assert call(params(**over)) == -1 and word in L.trhip_last_error(ctx._h), over
    # the parameter block before trhip_render_path's refusals, those before the environment's
    assert call(params(scale=-1.0), spp=0, env_h=None) == -1 and b"scale" in L.trhip_last_error(ctx._h)
    assert call(params(), spp=0, env_h=None) == -1 and b"spp" in L.trhip_last_error(ctx._h)
    assert call(params(), depth=0, env_h=None) == -1 and b"max_depth" in L.trhip_last_error(ctx._h)
    assert call(None) == -1 and call(params(), outp=None) == -1 and call(params(), scene_h=None) == -1 and call(params(), sensor=None) == -1 and call(params(), context=None) == -1
    assert call(params(), env_h=None) == -1 and b"null environment" in L.trhip_last_error(ctx._h)
    assert call(params(scale=3.0e38)) == -1 and b"+Inf" in L.trhip_last_error(ctx._h)  # 3e38 * (a texel of about 4) overflows
    assert L.trhip_render_path_env_device(ctx._h, flat._h, C.byref(sn), 1, 3, SEED, 0, h_env, C.byref(params()), None, C.byref(st)) == -1
    raw = C.c_void_p()
    ctx.check(L.trhip_scene_new(ctx._h, C.byref(raw)))
    try:
        assert call(params(), scene_h=raw, env_h=None) == -1 and b"not committed" in L.trhip_last_error(ctx._h)
    finally:
        L.trhip_scene_free(raw)
    holes = tgs.materialless(T)  # material-less primitives: trhip_render_path's refusal, before the environment is looked at
    assert call(params(), scene_h=holes.flatten()._h, env_h=None) == -3 and b"material-less" in L.trhip_last_error(ctx._h)
    other = T.Context(0)  # a second context on the same GPU: its environments are not this context's
    try:
        foreign = env._handle(other)
        assert call(params(), env_h=foreign) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        assert call(params(scale=3.0e38), env_h=foreign) == -1 and b"another context" in L.trhip_last_error(ctx._h), "the context before the scale"
        assert call(params()) == 0
        assert L.trhip_path_env_relight(ctx._h, foreign, C.byref(params()), T._ffi.fptr(out)) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        assert L.trhip_path_env_relight(ctx._h, None, C.byref(params()), T._ffi.fptr(out)) == -1 and b"null environment" in L.trhip_last_error(ctx._h)
        assert L.trhip_path_env_relight(ctx._h, h_env, C.byref(params(scale=3.0e38)), T._ffi.fptr(out)) == -1 and b"+Inf" in L.trhip_last_error(ctx._h)
        assert L.trhip_path_env_relight(ctx._h, h_env, C.byref(params()), None) == -1
        assert L.trhip_path_env_relight(ctx._h, h_env, C.byref(params()), T._ffi.fptr(out)) == 0, "a refused relight leaves the frame valid"
    finally:
        env.close()
        other.close()
    integ = T.PathIntegrator(cam, T.SeededSampler(1, seed=SEED), 3)
    with pytest.raises(T.TraceHipError, match="sample_map"):
        integ.render(scene, environment=sky_map(T), sample_map=T.SampleMap(np.ones((3, 5), np.uint32), 1))
    black = T.Environment.constant((0, 0, 0))
    assert call(params(scale=0.0), env_h=black._handle(ctx)) == 0  # a black sky at scale 0: allowed
    black.close()
