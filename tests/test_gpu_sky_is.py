"""Importance sampling of the environment map and the importance-sampled sky frame on the GPU (trhip_env_sample, trhip_env_pdf, trhip_render_sky_is;
docs/design/27-sky-importance.md), bit for bit against the model of tests/sky_is_model.py: the sampler on the u set (corners, table entries and their Float32 neighbours,
random points) and the density on tests/test_gpu_sky.py's direction set plus the sampled directions, at n = 1, 2, 7 and 64 under the identity and a turned matrix; the
per-sample radiance of the frame and its film on three scenes, two frame sizes, three mixes, both flags, two scales and two reaches, under a map with a bright texel in
each hemisphere; the frames around an importance-sampled frame on the same context; the device variant, shards, the denoiser and the refusals that need a context.

Shapes, scenes and cameras are tests/test_gpu_sky.py's.  Every test calls an entry point that this feature adds."""
import ctypes as C

import numpy as np
import pytest

import sky_is_model as im
import sky_model as sm
import test_gpu_sky as gs
from test_gpu_sky import assert_bits_equal, bits, camera, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
SEED, REACH, SIZES = gs.SEED, gs.REACH, gs.SIZES
MIXES = [0.25, 0.5, 15.0 / 16.0]
_cache = {}


def sun_env(T):
    """A 7 x 7 map of unequal texels with a bright texel in each hemisphere and rows without weight, under a turned matrix; its tables from the model."""
    if "env" not in _cache:
        t = im.test_map(7)
        _cache["env"] = (T.Environment(t, sm.rotation()), im.tables(t))
    return _cache["env"]


# ---- the sampler and the density ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_env_sample_and_pdf_equal_the_model(T, ctx, n, turned):
    R = sm.rotation() if turned else None
    t = im.test_map(n)
    tab = im.tables(t)
    u = im.u_set(tab)
    assert u.min() == 0 and u.max() == im.ONE_MINUS and u.shape[0] > 2000
    env = T.Environment(t, R)
    got = env.sample(u, ctx)
    ref, i, j, _, _ = im.env_sample(tab, u[:, 0], u[:, 1], R, cells=True)
    assert got.shape == (u.shape[0], 3)
    assert_bits_equal(got, ref, f"trhip_env_sample, n = {n}")
    empty = np.flatnonzero(tab.w.sum(axis=1) == 0)
    assert (empty.size > 0) == (n >= 7) and not np.isin(j, empty).any(), "rows without weight are in the map from n = 7 on, and are never chosen"
    inf, nan = np.inf, np.nan
    none = F([[0, 0, 0], [-0.0, 0, -0.0], [inf, 0, 0], [0, -inf, 1], [inf, inf, -inf], [nan, 0, 1], [1, nan, 0], [0, 1, nan], [nan, nan, nan], [3e38, 3e38, 3e38]])
    dirs = np.concatenate([sm.adversarial_directions(1000), none, sm.centre_directions(n).reshape(-1, 3), ref])
    p = env.pdf(dirs, ctx)
    assert p.shape == (dirs.shape[0],)
    assert_bits_equal(p, im.env_pdf(tab, dirs, R), f"trhip_env_pdf, n = {n}")
    assert not bits(p[1000:1010]).any(), "zero, Inf and NaN directions have density +0"
    assert (p[-ref.shape[0]:] > 0).all(), "every sampled direction has a positive density"
    assert env.sample(np.zeros((0, 2), F), ctx).shape == (0, 3) and env.pdf(np.zeros((0, 3), F), ctx).shape == (0,)
    L = T.lib()
    ctx.check(L.trhip_env_make_sampler(ctx._h, env._handle(ctx)))  # idempotent
    assert_bits_equal(env.sample(u[:64], ctx), ref[:64], "after a second trhip_env_make_sampler")
    env.close()


# ---- the frame --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["5x3-1spp", "37x29-3spp"])
@pytest.mark.parametrize("which", sorted(gs.SCENES))
def test_sample_radiance_and_film_equal_the_model(T, ob, ctx, which, small):
    scene, osc = scene_of(T, ob, which)
    cam, spp = camera(T, small), 1 if small else 3
    env, tab = sun_env(T)
    base = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=SEED)).samples(scene)
    sn = cam.sensor()
    seen = set()
    for mix in MIXES:
        for reach in (np.inf, REACH):
            tr = im.trace(osc, cam, spp, SEED, env.texels, env.world_to_env, mix=mix, max_distance=reach, tab=tab)
            assert tr.cls.shape == ((1, 3, 5) if small else (3, 31, 39))
            seen |= set(np.unique(tr.cls))
            if not small:
                share = [float((tr.cls == k).mean()) for k in (im.MISS, im.OCCLUDED, im.OPEN, im.NO_RAY)]
                print(f"{which}, mix {mix}, reach {reach}: model classes miss / occluded / open / no ray = " + " / ".join(f"{s:.3f}" for s in share))
                assert min(share[:3]) >= 0.04 and share[3] > 0, "misses, occluded, open rays and hits without a ray are all in the model's frame"
            n_rays = int(((tr.cls == im.OCCLUDED) | (tr.cls == im.OPEN)).sum())
            for scale in (0.0, 0.5):
                for albedo in (False, True):
                    for hide in (False, True):
                        what = f"{which}, mix {mix}, reach {reach}, scale {scale}, albedo {albedo}, hide_background {hide}"
                        ref = im.shade(tr, scale, base["albedo"].reshape(-1, 3) if albedo else None, hide)
                        integ = T.SkyIntegrator(cam, T.SeededSampler(spp, seed=SEED), env, max_distance=reach, albedo=albedo, scale=scale, hide_background=hide, importance=mix)
                        xyzw = integ.render(scene)
                        L = integ.sample_radiance(scene)
                        assert_bits_equal(L, ref.L, "per-sample radiance: " + what)
                        film = np.empty_like(xyzw)
                        ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, SEED, 0, T._ffi.fptr(np.ascontiguousarray(L)), T._ffi.fptr(film)))
                        assert_bits_equal(xyzw, film, "film vs trhip_film_accumulate: " + what)
                        if scale == 0.0:
                            assert not bits(L).any()
                        elif not small:
                            assert len(np.unique(L[ref.cls == im.OPEN], axis=0)) > 50, "the open rays read the map"
                        st = integ.stats
                        assert st.shadow_rays == n_rays and st.camera_samples == st.closest_rays == tr.cls.size
                        assert (st.launches_raygen, st.launches_trace_closest, st.launches_shade, st.launches_trace_any, st.launches_film) == (1, 1, 1, 1, 1)
    assert {im.MISS, im.OPEN} <= seen


def test_frames_around_an_importance_sampled_frame_keep_their_bits(T, ob, ctx):
    """trhip_render_sky, trhip_render_ao and trhip_render_path on the same context, before and after an importance-sampled frame."""
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    env, _ = sun_env(T)
    sky = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, scale=0.5, albedo=True)
    ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), albedo=True, background=0.25)
    path = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 4)

    def all_three():
        out = []
        for integ in (sky, ao, path):
            out.append(integ.render(scene).copy())
            out.append(integ.sample_radiance(scene))
        return out

    before = all_three()
    is_frame = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, scale=0.5, albedo=True, importance=True)
    assert is_frame.is_params.mix == 0.5
    got = is_frame.render(scene)
    assert got.any() and not np.array_equal(bits(got), bits(before[0])), "the importance-sampled frame is another estimator"
    for g, r, what in zip(all_three(), before, ("sky film", "sky samples", "AO film", "AO samples", "path film", "path samples")):
        assert_bits_equal(g, r, what + " after an importance-sampled frame")


def test_determinism_device_variant_and_shards(T, ob, ctx):
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    env, _ = sun_env(T)
    integ = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, importance=0.25)
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
    shards, films = [], []
    for spp, off in ((2, 0), (1, 2)):
        s = T.SkyIntegrator(cam, T.SeededSampler(spp, seed=SEED, sample_offset=off), env, importance=0.25)
        films.append(s.render(scene).astype(np.float64))
        shards.append(s.sample_radiance(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")
    # the film is additive over shards: the sum of the shard films is the whole film up to the Float32 rounding of either accumulation
    # (a film value sums fewer than 128 weighted samples: 128 roundings of 2^-24 each, relative to the largest value)
    assert np.abs(films[0] + films[1] - a).max() <= 2.0 ** -17 * float(np.abs(a).max())
    assert_bits_equal(cam.film.filter_weight_sum, integ.render(scene)[..., 3], "the film object holds the frame")


def test_film_passes_through_the_denoiser(T, ob, ctx):
    import denoise_model as dm
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    env, _ = sun_env(T)
    xyzw = T.SkyIntegrator(cam, T.SeededSampler(3, seed=SEED), env, importance=True).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(3, seed=SEED)).render(scene).planes
    assert_bits_equal(xyzw[..., 3], planes[..., 0, 3], "the film carries the planes' weights")
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
    err = lambda: L.trhip_last_error(ctx._h)
    env = T.Environment(sm.random_map(2))
    h_env = env._handle(ctx)  # no sampler yet

    def params(**over):
        p = T._ffi.SkyIsParams()
        assert L.trhip_sky_is_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=1, env_h=h_env, context=ctx._h):
        return L.trhip_render_sky_is(context, flat._h, C.byref(sn), spp, SEED, 0, env_h, C.byref(p), T._ffi.fptr(out), C.byref(st))

    u, d, o3, o1 = np.zeros((1, 2), F), np.ones((1, 3), F), np.zeros((1, 3), F), np.zeros(1, F)
    assert call(params()) == -1 and b"no sampler" in err()
    assert L.trhip_env_sample(ctx._h, h_env, T._ffi.fptr(u), 1, T._ffi.fptr(o3)) == -1 and b"no sampler" in err()
    assert L.trhip_env_pdf(ctx._h, h_env, T._ffi.fptr(d), 1, T._ffi.fptr(o1)) == -1 and b"no sampler" in err()
    assert L.trhip_env_make_sampler(ctx._h, None) == -1 and L.trhip_env_make_sampler(None, h_env) == -1
    assert L.trhip_env_make_sampler(ctx._h, h_env) == 0 and L.trhip_env_make_sampler(ctx._h, h_env) == 0
    assert call(params()) == 0 and out.any()
    assert L.trhip_env_sample(ctx._h, h_env, None, 1, T._ffi.fptr(o3)) == -1 and L.trhip_env_pdf(ctx._h, h_env, T._ffi.fptr(d), 1, None) == -1
    # the sky frame's refusals keep their order in front of the new ones
    for over, word in ((dict(max_distance=0.0), b"max_distance"), (dict(scale=-0.5), b"scale"), (dict(flags=4), b"flag"), (dict(mix=0.0), b"mix"), (dict(mix=1.0), b"mix"),
                       (dict(mix=float("nan")), b"mix")):
        assert call(params(**over)) == -1 and word in err(), over
    assert call(params(), spp=0) == -1 and b"spp" in err()
    assert call(params(), env_h=None) == -1 and b"null environment" in err()
    assert call(params(scale=3.0e38)) == -1 and b"+Inf" in err() and b"mix" not in err()  # the sky frame's own overflow: 3e38 * (a texel of about 4)
    assert env.texels.max() > 2.0 and env.texels.max() < 4.0
    assert call(params(scale=4.0e37, mix=15.0 / 16.0)) == -1 and b"1 - mix" in err()  # at most 1.6e38: finite, times 16 it is not, times 2 it is
    assert call(params(scale=4.0e37, mix=0.5)) == 0
    other = T.Context(0)  # a second context on the same GPU: its environments are not this context's
    try:
        foreign = env._sampler_handle(other)
        assert call(params(), env_h=foreign) == -1 and b"another context" in err()
        assert L.trhip_env_make_sampler(ctx._h, foreign) == -1 and b"another context" in err()
        assert L.trhip_env_sample(ctx._h, foreign, T._ffi.fptr(u), 1, T._ffi.fptr(o3)) == -1 and b"another context" in err()
        assert L.trhip_env_pdf(ctx._h, foreign, T._ffi.fptr(d), 1, T._ffi.fptr(o1)) == -1 and b"another context" in err()
        assert L.trhip_env_sample(other._h, foreign, T._ffi.fptr(u), 1, T._ffi.fptr(o3)) == 0
    finally:
        env.close()
        other.close()
    # a matrix that is not orthonormal: a scale of 1.001 is off by 2e-3, a Float32 rotation by 1e-7
    scaled = T.Environment(sm.random_map(2), (sm.rotation().astype(np.float64) * 1.001).astype(F))
    assert L.trhip_env_make_sampler(ctx._h, scaled._handle(ctx)) == -1 and b"orthonormal" in err()
    assert scaled.eval(d, ctx).any(), "the lookup keeps accepting any finite matrix"
    with pytest.raises(T.TraceHipError):
        scaled.sample(u, ctx)
    scaled.close()
    black = T.Environment.constant((0, 0, 0))
    assert L.trhip_env_make_sampler(ctx._h, black._handle(ctx)) == -1 and b"zero" in err()
    with pytest.raises(T.TraceHipError):
        T.SkyIntegrator(cam, T.SeededSampler(1, seed=SEED), black, importance=True).render(scene)
    black.close()
