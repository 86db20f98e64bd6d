"""The environment map and the sky-lit frame on the GPU (trhip_env_eval, trhip_render_sky; docs/design/25-sky.md), bit for bit against the model of tests/sky_model.py: the
lookup on the adversarial direction set; the per-sample radiance of the frame and its film (trhip_film_accumulate of those samples) on three scenes, two frame sizes, both
flags, two scales and two reaches; the anchor through existing code (a constant white map is trhip_render_ao with background 1, HIDE_BACKGROUND is background 0); the frames
around a sky frame on the same context; the device variant, shards, the denoiser and the refusals that need a context.

Shapes: a 5 x 3 crop under a filter of radius 1/2 at 1 spp (the sample bounds are the crop: 15 samples, fewer than one wave, misses among them) and 37 x 29 under the default Lanczos filter at
3 spp (39 x 31 x 3 = 3627 samples: 56 full waves and a partial one).  The classes of the larger frame are asserted from the model, never from the library's output."""
import ctypes as C

import numpy as np
import pytest

import ao_model as am
import sky_model as sm

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 0x5C1
REACH = 0.3  # tests/test_gpu_ao.py's finite reach: in the model it opens a third of the rays that an infinite reach finds occluded
SIZES = [1, 2, 7, 64]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def camera(T, small=False):
    """37 x 29 under the default filter, or a 5 x 3 crop of it under a filter of radius 1/2, placed over the right end of the floor's edge: camera misses, occluded and open
    rays all lie inside it (the model's classes; the test asserts it)."""
    crop = T.Bounds2([30.2 / 37, 22.2 / 29], [35.2 / 37, 25.2 / 29]) if small else T.Bounds2([0.0, 0.0], [1.0, 1.0])
    flt = T.LanczosSincFilter([0.5, 0.5], 3.0) if small else T.LanczosSincFilter([1.0, 1.0], 3.0)
    film = T.Film([37, 29], crop, flt, 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def materialless(T):
    """tests/test_gpu_ao.py's variant of the Cornell box: the floor quad has no material, the glass sphere's Kt is black."""
    prims, _ = T.scenes.cornell_primitives()
    prims[0] = T.GeometricPrimitive(prims[0].shape, None)
    prims[1] = T.GeometricPrimitive(prims[1].shape, None)
    glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(0.9, 0.8, 0.7)), T.ConstantTexture(T.RGBSpectrum(0.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)
    prims[-1] = T.GeometricPrimitive(prims[-1].shape, glass)
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


SCENES = {"cornell": lambda T: T.scenes.cornell_scene(), "mesh": lambda T: T.scenes.mesh_scene(16), "materialless": materialless}
_cache = {}


def scene_of(T, ob, which):
    """(scene, oracle scene on the committed tree), built once per module and left alone."""
    if which not in _cache:
        scene = SCENES[which](T)
        _cache[which] = (scene, ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh()))
    return _cache[which]


def ao_frame(T, ob, which, small, reach):
    """The AO model's frame (samples, hits, occlusion rays, verdicts): computed once per (scene, size, reach) and shared."""
    key = (which, small, float(reach))
    if key not in _cache:
        spp = 1 if small else 3
        _cache[key] = am.render(scene_of(T, ob, which)[1], camera(T, small), spp, SEED, max_distance=reach)
    return _cache[key]


def sky_map(T):
    """A 7 x 7 map of unequal texels under a turned matrix: every sample reads its own blend."""
    if "env" not in _cache:
        _cache["env"] = T.Environment(sm.random_map(7), sm.rotation())
    return _cache["env"]


# ---- the lookup ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_env_eval_equals_the_model(T, ctx, n, turned):
    inf, nan = np.inf, np.nan
    none = F([[0, 0, 0], [-0.0, 0, -0.0], [inf, 0, 0], [0, -inf, 1], [inf, inf, -inf], [nan, 0, 1], [1, nan, 0], [0, 1, nan], [nan, nan, nan], [3e38, 3e38, 3e38]])
    dirs = np.concatenate([sm.adversarial_directions(1000), none, sm.centre_directions(n).reshape(-1, 3)])
    R = sm.rotation() if turned else None
    t = sm.random_map(n)
    env = T.Environment(t, R)
    got = env.eval(dirs, ctx)
    assert got.shape == dirs.shape
    assert_bits_equal(got, sm.env_eval(t, dirs, R), f"trhip_env_eval, n = {n}")
    assert not bits(got[1000:1010]).any(), "zero, Inf and NaN directions return +0"
    size = C.c_uint32(0)
    ctx.check(T.lib().trhip_env_size(env._handle(ctx), C.byref(size)))
    assert size.value == n
    flat = T.Environment(np.broadcast_to(F([0.1, 1.7, 3.0e-5]), (n, n, 3)), R)
    assert_bits_equal(flat.eval(dirs[:1000], ctx), np.broadcast_to(F([0.1, 1.7, 3.0e-5]), (1000, 3)), "a constant map returns its constant")
    env.close()
    flat.close()
    assert T.Environment.constant((1, 2, 3)).eval(np.zeros((0, 3), F), ctx).shape == (0, 3)  # no directions: nothing to do


# ---- the frame --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["5x3-1spp", "37x29-3spp"])
@pytest.mark.parametrize("which", sorted(SCENES))
def test_sample_radiance_and_film_equal_the_model(T, ob, ctx, which, small):
    scene, osc = scene_of(T, ob, which)
    cam, spp, env = camera(T, small), 1 if small else 3, sky_map(T)
    assert tuple(cam.film.size) == ((3, 5) if small else (29, 37))
    base = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=SEED)).samples(scene)
    if which == "materialless":
        assert small or ((base["material"] == -1) & (base["prim"] >= 0)).mean() > 0.05, "the primitives without a material are in view"
    sn = cam.sensor()
    for reach in (np.inf, REACH):
        frame = ao_frame(T, ob, which, small, reach)
        assert frame.cls.shape == ((1, 3, 5) if small else (3, 31, 39))
        if small:
            assert set(np.unique(frame.cls)) == {am.MISS, am.OCCLUDED, am.OPEN}, "the crop holds all three classes in the model"
        else:
            miss, occluded, opened = am.shares(frame.cls)
            print(f"{which}, reach {reach}: model classes miss / occluded / open = {miss:.3f} / {occluded:.3f} / {opened:.3f}")
            assert min(miss, occluded, opened) >= 0.05, "camera misses, occluded and open rays each hold 5 % of the samples in the model"
        for scale in (0.0, 0.5):
            for albedo in (False, True):
                for hide in (False, True):
                    what = f"{which}, reach {reach}, scale {scale}, albedo {albedo}, hide_background {hide}"
                    ref = sm.render(osc, cam, spp, SEED, env.texels, env.world_to_env, max_distance=reach, scale=scale, albedo=base["albedo"].reshape(-1, 3) if albedo else None,
                                    hide_background=hide, frame=frame)
                    integ = T.SkyIntegrator(cam, T.SeededSampler(spp, seed=SEED), env, max_distance=reach, albedo=albedo, scale=scale, hide_background=hide)
                    xyzw = integ.render(scene)
                    L = integ.sample_radiance(scene)
                    assert_bits_equal(L, ref.L, "per-sample radiance: " + what)
                    film = np.empty_like(xyzw)
                    ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, SEED, 0, T._ffi.fptr(np.ascontiguousarray(L)), T._ffi.fptr(film)))
                    assert_bits_equal(xyzw, film, "film vs trhip_film_accumulate: " + what)
                    if scale == 0.0:
                        assert not bits(L).any()
                    elif not small:
                        assert len(np.unique(L[ref.cls == sm.OPEN], axis=0)) > 50, "the open rays read the map"
                        assert hide or len(np.unique(L[ref.cls == sm.MISS], axis=0)) > 50, "the misses read the map"
                    st = integ.stats
                    assert st.shadow_rays == int(frame.hit.sum()) and st.camera_samples == st.closest_rays == frame.cls.size
                    assert st.n_batches == 1 and st.max_depth_reached == 1
                    assert (st.launches_raygen, st.launches_trace_closest, st.launches_shade, st.launches_trace_any, st.launches_film) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize("albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("which", ["mesh", "materialless"])
def test_a_constant_white_map_is_the_ao_frame(T, ob, ctx, which, albedo):
    """The anchor through existing code: Environment.constant((1, 1, 1)) with scale 1 is trhip_render_ao with background 1, film and samples, bit for bit; HIDE_BACKGROUND is
    background 0."""
    scene, _ = scene_of(T, ob, which)
    cam, white = camera(T), T.Environment.constant((1, 1, 1))
    for reach in (np.inf, REACH):
        for hide in (False, True):
            ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), max_distance=reach, albedo=albedo, background=0.0 if hide else 1.0)
            ao_film = ao.render(scene)
            ao_L = ao.sample_radiance(scene)
            sky = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), white, max_distance=reach, albedo=albedo, hide_background=hide)
            sky_film = sky.render(scene)
            assert_bits_equal(sky.sample_radiance(scene), ao_L, f"samples, reach {reach}, hide_background {hide}")
            assert_bits_equal(sky_film, ao_film, f"film, reach {reach}, hide_background {hide}")
            assert ao_L.any() and (hide or (ao_L == 1).all(axis=-1).mean() > 0.05)


def test_frames_around_a_sky_frame_keep_their_bits(T, ob, ctx):
    """trhip_render_ao and trhip_render_path on the same context, before and after a sky frame."""
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), albedo=True, background=0.25)
    path = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 4)

    def both():
        a = ao.render(scene).copy()
        aL = ao.sample_radiance(scene)
        p = path.render(scene).copy()
        return a, aL, p, path.sample_radiance(scene)

    before = both()
    sky = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), sky_map(T), scale=0.5)
    assert sky.render(scene).any()
    for got, ref, what in zip(both(), before, ("AO film", "AO samples", "path film", "path samples")):
        assert_bits_equal(got, ref, what + " after a sky frame")


def test_determinism_device_variant_and_shards(T, ob, ctx):
    scene, _ = scene_of(T, ob, "mesh")
    cam, env = camera(T), sky_map(T)
    integ = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env)
    a = integ.render(scene)
    La = integ.sample_radiance(scene)
    assert_bits_equal(integ.render(scene), a, "film, two calls")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples, two calls")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.render(scene, device_out=d_film.ptr) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), a, "device variant")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples after the device variant")
    d_film.free()
    shards = []
    for spp, off in ((2, 0), (1, 2)):
        s = T.SkyIntegrator(cam, T.SeededSampler(spp, seed=SEED, sample_offset=off), env)
        s.render(scene)
        shards.append(s.sample_radiance(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")
    assert_bits_equal(cam.film.filter_weight_sum, integ.render(scene)[..., 3], "the film object holds the frame")


def test_film_passes_through_the_denoiser(T, ob, ctx):
    import denoise_model as dm
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    xyzw = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), sky_map(T)).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(3, seed=SEED)).render(scene).planes
    assert_bits_equal(xyzw[..., 3], planes[..., 0, 3], "the sky film carries the planes' weights")
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    p = d.params
    prm = dm.Params(p.sigma_colour, p.sigma_normal, p.sigma_plane, iterations=p.iterations, demodulate=bool(p.flags & 1), albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)
    surface = dm.surface_mask(xyzw, planes, prm)
    assert surface.sum() > 50 and (~surface).sum() > 20
    assert_bits_equal(out[~surface], xyzw[~surface], "non-surface pixels (the sky among them) pass through")
    assert_bits_equal(out, dm.denoise(xyzw, planes, prm), "the denoiser's model")


def test_refusals_with_a_context(T, ob, ctx):
    scene, _ = scene_of(T, ob, "cornell")
    flat, cam, L = scene.flatten(), camera(T, True), T.lib()
    sn, st, out = cam.sensor(), T.Stats(), np.zeros((3, 5, 4), F)
    env = T.Environment(sm.random_map(2))
    h_env = env._handle(ctx)

    def params(**over):
        p = T._ffi.SkyParams()
        assert L.trhip_sky_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=1, scene_h=flat._h, sensor=sn, outp=T._ffi.fptr(out), context=ctx._h, env_h=h_env):
        return L.trhip_render_sky(context, scene_h, C.byref(sensor) if sensor is not None else None, spp, SEED, 0, env_h, C.byref(p) if p is not None else None, outp, C.byref(st))

    assert call(params()) == 0 and out.any()
    for over, word in ((dict(max_distance=float("nan")), b"max_distance"), (dict(max_distance=0.0), b"max_distance"), (dict(max_distance=-1.0), b"max_distance"),
                       (dict(scale=-0.5), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"), (dict(flags=4), b"flag"), (dict(reserved=9), b"reserved")):
        assert call(params(**over)) == -1 and word in L.trhip_last_error(ctx._h), over
    assert call(params(), spp=0) == -1 and b"spp" in L.trhip_last_error(ctx._h)
    assert call(None) == -1 and call(params(), outp=None) == -1 and call(params(), scene_h=None) == -1 and call(params(), sensor=None) == -1 and call(params(), context=None) == -1
    assert call(params(), env_h=None) == -1 and b"null environment" in L.trhip_last_error(ctx._h)
    assert call(params(scale=3.0e38)) == -1 and b"+Inf" in L.trhip_last_error(ctx._h)  # 3e38 * (a texel of about 4) overflows
    assert L.trhip_render_sky_device(ctx._h, flat._h, C.byref(sn), 1, SEED, 0, h_env, C.byref(params()), None, C.byref(st)) == -1
    raw = C.c_void_p()
    ctx.check(L.trhip_scene_new(ctx._h, C.byref(raw)))
    try:
        assert call(params(), scene_h=raw) == -1 and b"not committed" in L.trhip_last_error(ctx._h)
    finally:
        L.trhip_scene_free(raw)
    other = T.Context(0)  # a second context on the same GPU: its environments are not this context's
    try:
        foreign = env._handle(other)
        assert call(params(), env_h=foreign) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        d = np.ones((1, 3), F)
        assert L.trhip_env_eval(ctx._h, foreign, T._ffi.fptr(d), 1, T._ffi.fptr(d)) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        assert L.trhip_env_eval(other._h, foreign, T._ffi.fptr(d), 1, T._ffi.fptr(d)) == 0
    finally:
        env.close()
        other.close()
    black = T.Environment.constant((0, 0, 0))
    assert call(params(max_distance=1e-30, scale=0.0), env_h=black._handle(ctx)) == 0  # tiny but positive, and a black sky: allowed
    black.close()
