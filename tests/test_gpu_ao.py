"""The ambient-occlusion integrator (trhip_render_ao, AmbientOcclusionIntegrator) on the GPU: per-sample radiance against the oracle-only model of tests/ao_model.py bit for bit
on four scenes (spheres and triangles, a hierarchy, a one-leaf accelerator, a clipped sphere) and with a finite reach; the film against trhip_film_accumulate of those samples
and its weights against the path frame's, bit for bit; the albedo flag, the background, determinism, the device variant, shards, a scene without lights, the denoiser, the
statistics and the refusals.

Shapes: film 16 x 12 under the default Lanczos filter (the sample bounds, 18 x 14, leave partial 16 x 16 tiles), 3 samples per pixel (odd, more than one).  Camera and reach
were chosen with the model alone, without a GPU, so that misses, occluded and open samples each hold at least 5 % of every frame; the tests assert that from the model's
classes, never from the library's output."""
import ctypes as C

import numpy as np
import pytest

import ao_model as am

pytestmark = pytest.mark.gpu

F = np.float32
SPP, SEED = 3, 0xA0
REACH = 0.3  # the finite reach of the Cornell case: in the model it opens a third of the rays that an infinite reach finds occluded


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def camera(T, crop=None, resolution=(16, 12), position=(0, 15, 50), target=(0, 0, -2)):
    film = T.Film(list(resolution), T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(list(position), list(target), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def cornell_variant(T):
    """tests/test_gpu_aov.py's variant: the Cornell box (triangles and two spheres) with a floor quad that has no material and a glass sphere whose Kt is black."""
    prims, _ = T.scenes.cornell_primitives()
    prims[0] = T.GeometricPrimitive(prims[0].shape, None)
    prims[1] = T.GeometricPrimitive(prims[1].shape, None)
    glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(0.9, 0.8, 0.7)), T.ConstantTexture(T.RGBSpectrum(0.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)
    prims[-1] = T.GeometricPrimitive(prims[-1].shape, glass)
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


def clipped_sphere(T):
    """The box without its spheres and one sphere clipped in z and in phi (the kernels' general sphere test); no lights."""
    prims, white = T.scenes.cornell_primitives(False)
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.5, 0.3, -2.5]), False), 0.3, -0.1, 0.25, 270.0), white))
    return T.Scene([], T.BVHAccel(prims, 1))


SCENES = {
    "cornell_variant": cornell_variant,                # (a) spheres and triangles
    "mesh": lambda T: T.scenes.mesh_scene(16),         # (b) a hierarchy: the hybrid walk for the camera rays, the canonical any-hit path for the occlusion rays
    "shadows": lambda T: T.scenes.shadows_scene(),     # (c) eight primitives: a one-leaf accelerator
    "clipped_sphere": clipped_sphere,                  # (d)
}
CASES = [("cornell_variant", np.inf), ("cornell_variant", REACH), ("mesh", np.inf), ("shadows", np.inf), ("clipped_sphere", np.inf)]
_cache = {}


def scene_of(T, ob, which):
    """(scene, oracle scene on the committed tree), built once per module and left alone."""
    if which not in _cache:
        scene = SCENES[which](T)
        _cache[which] = (scene, ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh()))
    return _cache[which]


def model_of(T, ob, which, reach=np.inf, **kw):
    key = (which, float(reach), tuple(sorted(kw.items())))
    if key not in _cache:
        scene, osc = scene_of(T, ob, which)
        _cache[key] = am.render(osc, camera(T), SPP, SEED, max_distance=reach, **kw)
    return _cache[key]


def ao(T, cam=None, spp=SPP, offset=0, **kw):
    return T.AmbientOcclusionIntegrator(cam or camera(T), T.SeededSampler(spp, seed=SEED, sample_offset=offset), **kw)


@pytest.mark.parametrize("which,reach", CASES, ids=[f"{w}-{r}" for w, r in CASES])
def test_sample_radiance_equals_the_model(T, ob, ctx, which, reach):
    scene, _ = scene_of(T, ob, which)
    ref = model_of(T, ob, which, reach)
    miss, occluded, opened = am.shares(ref.cls)
    print(f"{which}, reach {reach}: kernel {scene.flatten().closest_kernel_name()}, model classes miss / occluded / open = {miss:.3f} / {occluded:.3f} / {opened:.3f}")
    assert min(miss, occluded, opened) >= 0.05, "each class must hold 5 % of the samples in the model"
    if which == "mesh":
        assert "leaf" not in scene.flatten().closest_kernel_name(), "this case is the hierarchy"
    if which == "shadows":
        assert "leaf" in scene.flatten().closest_kernel_name(), "this case is the one-leaf scene"
    if which == "clipped_sphere":
        flat = scene.flatten()
        _, prim, _, _ = scene_of(T, ob, which)[1].trace_closest(ref.rays)
        on_sphere = flat.bvh()[3][np.where(prim >= 0, prim, 0)] == len(flat.bvh()[3]) - 1
        assert (on_sphere & (prim >= 0)).sum() >= 10, "the clipped sphere is in view"
    if np.isfinite(reach):
        far = model_of(T, ob, which, np.inf)
        assert ((far.cls == am.OCCLUDED) & (ref.cls == am.OPEN)).sum() >= 0.05 * ref.hit.sum(), "the finite reach must change the verdict of 5 % of the hitting samples"
    integ = ao(T, max_distance=reach)
    xyzw = integ.render(scene)
    L = integ.sample_radiance(scene)
    assert L.shape == ref.L.shape == (SPP, 14, 18, 3)
    assert_bits_equal(L, ref.L, "per-sample radiance")
    assert np.isfinite(xyzw).all()
    st = integ.stats
    assert st.shadow_rays == int(ref.hit.sum()) and st.camera_samples == st.closest_rays == ref.cls.size
    assert st.n_batches == 1 and st.max_depth_reached == 1 and st.fallback_rays <= st.closest_rays and st.ms_total > 0
    assert (st.launches_raygen, st.launches_trace_closest, st.launches_shade, st.launches_trace_any, st.launches_film) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize("crop", [None, ([0.2, 0.1], [0.9, 0.7])], ids=["full", "cropped"])
def test_film_is_film_accumulate_of_the_samples(T, ob, ctx, crop):
    scene = T.scenes.cornell_scene()
    cam = camera(T, crop)
    if crop:
        assert tuple(cam.film.crop_bounds.p_min) != (1.0, 1.0)
    integ = ao(T, cam)
    xyzw = integ.render(scene)
    L = integ.sample_radiance(scene)
    assert 0.05 < (L == 1).mean() < 0.95
    sn, ref = cam.sensor(), np.empty_like(xyzw)
    ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), SPP, SEED, 0, T._ffi.fptr(np.ascontiguousarray(L)), T._ffi.fptr(ref)))
    assert_bits_equal(xyzw, ref, "film vs trhip_film_accumulate")
    path = T.PathIntegrator(cam, T.SeededSampler(SPP, seed=SEED), 1).render(scene)
    assert np.abs(path[..., 3]).min() > 0
    assert_bits_equal(xyzw[..., 3], path[..., 3], "weights vs the path frame's filter_weight_sum")


def test_albedo_flag(T, ob, ctx):
    """L = v * base colour, v from the model, the base colour from trhip_render_aov's records of the same samples.  The scene has two triangles without a material."""
    scene, _ = scene_of(T, ob, "cornell_variant")
    ref = model_of(T, ob, "cornell_variant")
    rec = T.AOVIntegrator(camera(T), T.SeededSampler(SPP, seed=SEED)).samples(scene)
    assert ((rec["material"] == -1) & (rec["prim"] >= 0)).any(), "a primitive without a material is in view"
    v = (ref.cls == am.OPEN).astype(F)[..., None]
    integ = ao(T, albedo=True)
    integ.render(scene)
    L = integ.sample_radiance(scene)
    assert_bits_equal(L, v * rec["albedo"], "v * albedo")
    assert len(np.unique(L[ref.cls == am.OPEN], axis=0)) >= 3, "several base colours are in view"
    assert not L[(ref.cls == am.OPEN) & (rec["material"] == -1)].any()
    again = am.render(scene_of(T, ob, "cornell_variant")[1], camera(T), SPP, SEED, albedo=rec["albedo"].reshape(-1, 3))
    assert_bits_equal(L, again.L, "the model with the base colours")


def test_background(T, ob, ctx):
    scene, _ = scene_of(T, ob, "cornell_variant")
    ref = model_of(T, ob, "cornell_variant")
    plain, lit = ao(T), ao(T, background=0.25)
    plain.render(scene)
    L0 = plain.sample_radiance(scene)
    lit.render(scene)
    L1 = lit.sample_radiance(scene)
    miss = ref.cls == am.MISS
    assert miss.mean() >= 0.05
    assert np.all(L1[miss] == F(0.25)) and not L0[miss].any()
    assert_bits_equal(L1[~miss], L0[~miss], "hitting samples")
    assert_bits_equal(L1, model_of(T, ob, "cornell_variant", background=0.25).L, "the model with a background")


def test_determinism_device_variant_and_shards(T, ob, ctx):
    scene, _ = scene_of(T, ob, "mesh")
    cam = camera(T)
    integ = ao(T, cam)
    a = integ.render(scene)
    La = integ.sample_radiance(scene)
    b = integ.render(scene)
    Lb = integ.sample_radiance(scene)
    assert_bits_equal(a, b, "film, two calls")
    assert_bits_equal(La, Lb, "samples, two calls")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.render(scene, device_out=d_film.ptr) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), a, "device variant")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples after the device variant")
    d_film.free()
    shards = []
    for spp, off in ((2, 0), (1, 2)):
        s = ao(T, cam, spp, off)
        s.render(scene)
        shards.append(s.sample_radiance(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")


def test_a_scene_without_lights_renders_through_call(T, ob, ctx):
    scene, _ = scene_of(T, ob, "clipped_sphere")
    assert scene.lights == []
    cam = camera(T)
    integ = ao(T, cam)
    assert not cam.film.xyz.any()
    assert integ(scene) is None  # no file name: nothing is saved
    assert_bits_equal(cam.film.filter_weight_sum, integ.render(scene)[..., 3], "film weights")
    assert (cam.film.xyz != 0).mean() > 0.2, "the film is filled"


def test_film_passes_through_the_denoiser(T, ob, ctx):
    import denoise_model as dm
    scene = T.scenes.mesh_scene(16)
    cam = camera(T, resolution=(32, 24), position=(5, 18, 50), target=(0.2, 0.2, -2.5))  # half of the samples miss (the model's count): whole regions of missing pixels
    xyzw = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(4, seed=SEED)).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(4, seed=SEED)).render(scene).planes
    assert_bits_equal(xyzw[..., 3], planes[..., 0, 3], "the AO film carries the planes' weights")
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    p = d.params
    prm = dm.Params(p.sigma_colour, p.sigma_normal, p.sigma_plane, iterations=p.iterations, demodulate=bool(p.flags & 1), albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)
    surface = dm.surface_mask(xyzw, planes, prm)
    missing = planes[..., 1, 3] == 0
    assert surface.sum() > 50 and missing.sum() > 20 and not (surface & missing).any()
    assert np.isfinite(out[surface]).all()
    assert_bits_equal(out[missing], xyzw[missing], "missing pixels")
    assert_bits_equal(out[~surface], xyzw[~surface], "non-surface pixels")
    assert (bits(out[surface]) != bits(xyzw[surface])).any(), "the filter must act"
    assert_bits_equal(out, dm.denoise(xyzw, planes, prm), "the denoiser's model")


def test_refusals_with_a_context(T, ob, ctx):
    scene, _ = scene_of(T, ob, "shadows")
    flat, cam = scene.flatten(), camera(T)
    sn, st, out, L = cam.sensor(), T.Stats(), np.zeros((12, 16, 4), F), T.lib()

    def params(**over):
        p = T._ffi.AoParams()
        assert L.trhip_ao_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=SPP, scene_h=flat._h, sensor=sn, outp=T._ffi.fptr(out), context=ctx._h):
        return L.trhip_render_ao(context, scene_h, C.byref(sensor) if sensor is not None else None, spp, SEED, 0, C.byref(p) if p is not None else None, outp, C.byref(st))

    assert call(params()) == 0 and out.any()
    for over, word in ((dict(max_distance=float("nan")), b"max_distance"), (dict(max_distance=0.0), b"max_distance"), (dict(max_distance=-1.0), b"max_distance"),
                       (dict(background=-0.5), b"background"), (dict(background=float("inf")), b"background"), (dict(background=float("nan")), b"background"),
                       (dict(flags=2), b"flag"), (dict(reserved=9), b"reserved")):
        assert call(params(**over)) == -1 and word in L.trhip_last_error(ctx._h), over
    assert call(params(), spp=0) == -1 and b"spp" in L.trhip_last_error(ctx._h)
    assert call(None) == -1 and call(params(), outp=None) == -1 and call(params(), scene_h=None) == -1 and call(params(), sensor=None) == -1 and call(params(), context=None) == -1
    assert L.trhip_render_ao_device(ctx._h, flat._h, C.byref(sn), SPP, SEED, 0, C.byref(params()), None, C.byref(st)) == -1
    raw = C.c_void_p()
    ctx.check(L.trhip_scene_new(ctx._h, C.byref(raw)))
    try:
        assert call(params(), scene_h=raw) == -1 and b"not committed" in L.trhip_last_error(ctx._h)
    finally:
        L.trhip_scene_free(raw)
    assert call(params(max_distance=1e-30)) == 0  # tiny but positive: allowed
