"""Adaptive sampling on the GPU (docs/design/24-adaptive.md), every comparison bit for bit.

Map frames (trhip_render_path_map): counts == spp against trhip_render_path; a seeded random map that holds zeros, an all-zero 16 x 16 tile, an all-zero run of 64 consecutive
sample pixels, one pixel at max_spp and a sum that is no multiple of 64 — drawn samples against the oracle's and the uniform frame's, the rest +0.0, the film against the
oracle-only model of tests/sample_map_model.py, stats.camera_samples; the same map in at least three batches; sample_offset 7; the _device variant; the refusals in the
header's order.  The statistics and map kernels against their numpy models on 1 x 1, 5 x 3, 37 x 29 and 64 x 64 sample pixels with NaN, +-Inf and zero records, and on both
record layouts of a real frame.  AdaptivePathIntegrator against the same calls made by hand.

Shapes: shadows_scene (a hierarchy), the Cornell box (the one-leaf accelerator), mesh_scene(16) (the two-tree hybrid walk); film 37 x 29 under the radius-1 filter (packed
records, several tiles, a partial group of 64 sample pixels) and under LanczosSincFilter([2.5, 1.5], 3) (sample-major records, the block gather); films 5 x 3 and 1 x 1;
max_spp 5, depth 4."""
import ctypes as C

import numpy as np
import pytest

import sample_map_model as sm

pytestmark = pytest.mark.gpu

F = np.float32
MAX_SPP, DEPTH, SEED = 5, 4, 0x5A
R1, WIDE = (1.0, 1.0), (2.5, 1.5)
SCENES = {"shadows": lambda T: T.scenes.shadows_scene(), "cornell": lambda T: T.scenes.cornell_scene(), "mesh16": lambda T: T.scenes.mesh_scene(16)}
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def assert_equal_up_to_nan_payload(got, ref, what):
    """Bit for bit, except that a NaN is any NaN: the sign and payload of a generated NaN (Inf - Inf) belong to the machine, not to the arithmetic."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaNs in other places"
    assert_bits_equal(np.where(np.isnan(ref), F(0), got), np.where(np.isnan(ref), F(0), ref), what)


def camera(T, resolution=(37, 29), radius=R1):
    film = T.Film(list(resolution), T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter(list(radius), 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def scene_of(T, which):
    if which not in _cache:
        _cache[which] = SCENES[which](T)
    return _cache[which]


def uniform(T, which, resolution, radius, offset=0):
    """(film, samples) of trhip_render_path at MAX_SPP: rendered once per case and left alone."""
    key = ("uniform", which, resolution, radius, offset)
    if key not in _cache:
        integ = T.PathIntegrator(camera(T, resolution, radius), T.SeededSampler(MAX_SPP, seed=SEED, sample_offset=offset), DEPTH)
        xyzw = integ.render(scene_of(T, which))
        _cache[key] = (xyzw, integ.sample_radiance(scene_of(T, which)))
    return _cache[key]


def oracle(T, ob, which, radius, offset=0):
    """(film, samples) of the oracle at MAX_SPP on the committed tree, 37 x 29."""
    key = ("oracle", which, radius, offset)
    if key not in _cache:
        scene = scene_of(T, which)
        osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh())
        xyzw, L, _ = osc.render(camera(T, (37, 29), radius), "path", MAX_SPP, DEPTH, seed=SEED, sample_offset=offset, want_samples=True)
        _cache[key] = (xyzw, L)
    return _cache[key]


def map_frame(T, which, resolution, radius, counts, offset=0, device=False):
    """(film, dense samples, stats) of a map frame."""
    cam = camera(T, resolution, radius)
    integ = T.PathIntegrator(cam, T.SeededSampler(MAX_SPP, seed=SEED, sample_offset=offset), DEPTH)
    m = T.SampleMap(counts, MAX_SPP)
    if device:
        h, w = cam.film.size
        buf = T._ffi.DeviceBuffer(h * w * 16)
        integ.render(scene_of(T, which), device_out=buf.ptr, sample_map=m)
        xyzw = buf.to_host(np.float32, (h, w, 4))
        buf.free()
    else:
        xyzw = integ.render(scene_of(T, which), sample_map=m)
    return xyzw, integ.sample_radiance(scene_of(T, which)), integ.stats


def random_map(T, radius):
    """The map of the module docstring for the 37 x 29 film, made from the shapes alone."""
    sbh, sbw, _, _ = sm.sample_shape(camera(T, (37, 29), radius))
    rng = np.random.default_rng(1234 + sbw)
    c = rng.integers(0, MAX_SPP + 1, (sbh, sbw)).astype(np.uint32)
    c[0:16, 16:32] = 0                 # the whole tile (0, 1)
    flat = c.reshape(-1)
    flat[768:832] = 0                  # the pixel group 12 of the pixel-group-major records
    flat[5] = MAX_SPP
    if int(flat.sum()) % 64 == 0:
        flat[6] = (flat[6] + 1) % (MAX_SPP + 1)
    assert (c == 0).any() and int(c.sum()) % 64 != 0 and c.max() == MAX_SPP and not c[0:16, 16:32].any() and not flat[768:832].any()
    return c


def check_map_frame(T, ob, which, radius, got, counts, offset=0):
    xyzw, L, stats = got
    ref_xyzw, ref_L = oracle(T, ob, which, radius, offset)
    _, uni_L = uniform(T, which, (37, 29), radius, offset)
    drawn = np.arange(MAX_SPP)[:, None, None] < counts[None]
    assert_bits_equal(L[drawn], ref_L[drawn], "drawn samples vs the oracle's")
    assert_bits_equal(L[drawn], uni_L[drawn], "drawn samples vs the uniform frame's")
    assert not bits(L[~drawn]).any(), "a sample that was not drawn is not +0.0"
    assert_bits_equal(xyzw, sm.film_model(ob, camera(T, (37, 29), radius), ref_L, counts, SEED, offset), "film vs the oracle model")
    assert stats.camera_samples == int(counts.sum())
    assert 0 < stats.closest_rays <= int(counts.sum()) * DEPTH


@pytest.mark.parametrize("resolution,radius", [((37, 29), R1), ((37, 29), WIDE), ((5, 3), R1), ((1, 1), R1)])
@pytest.mark.parametrize("which", list(SCENES))
def test_uniform_counts_are_render_path(T, ctx, which, resolution, radius):
    ref_xyzw, ref_L = uniform(T, which, resolution, radius)
    sbh, sbw, _, _ = sm.sample_shape(camera(T, resolution, radius))
    xyzw, L, stats = map_frame(T, which, resolution, radius, np.full((sbh, sbw), MAX_SPP))
    assert_bits_equal(L, ref_L, "samples")
    assert_bits_equal(xyzw, ref_xyzw, "film")
    assert stats.camera_samples == sbh * sbw * MAX_SPP


@pytest.mark.parametrize("radius", [R1, WIDE])
@pytest.mark.parametrize("which", list(SCENES))
def test_random_map(T, ob, ctx, which, radius):
    counts = random_map(T, radius)
    check_map_frame(T, ob, which, radius, map_frame(T, which, (37, 29), radius, counts), counts)


@pytest.mark.parametrize("radius", [R1, WIDE])
def test_random_map_in_three_batches(T, ob, ctx, radius):
    counts = random_map(T, radius)
    whole = map_frame(T, "mesh16", (37, 29), radius, counts)
    ctx.set_option("batch_paths", 512)
    try:
        got = map_frame(T, "mesh16", (37, 29), radius, counts)
    finally:
        ctx.set_option("batch_paths", 0)
    assert got[2].n_batches >= 3 and got[2].n_batches == -(-int(counts.sum()) // 512) and whole[2].n_batches == 1
    check_map_frame(T, ob, "mesh16", radius, got, counts)
    assert_bits_equal(got[0], whole[0], "film in batches vs in one")
    assert_bits_equal(got[1], whole[1], "samples in batches vs in one")


@pytest.mark.parametrize("radius", [R1, WIDE])
def test_sample_offset(T, ob, ctx, radius):
    counts = random_map(T, radius)
    check_map_frame(T, ob, "shadows", radius, map_frame(T, "shadows", (37, 29), radius, counts, offset=7), counts, offset=7)


@pytest.mark.parametrize("radius", [R1, WIDE])
def test_device_variant_is_the_host_variant(T, ctx, radius):
    counts = random_map(T, radius)
    host, dev = map_frame(T, "cornell", (37, 29), radius, counts), map_frame(T, "cornell", (37, 29), radius, counts, device=True)
    assert_bits_equal(dev[0], host[0], "film")
    assert_bits_equal(dev[1], host[1], "samples")
    assert dev[2].camera_samples == host[2].camera_samples == int(counts.sum())


def test_refusals_in_their_order(T, ctx):
    L = T.lib()
    scene = scene_of(T, "shadows")
    flat = scene.flatten(ctx)
    cam = camera(T, (5, 3))
    sn = cam.sensor()
    sbh, sbw, _, _ = sm.sample_shape(cam)
    out = np.zeros((3, 5, 4), F)
    d_out = T._ffi.DeviceBuffer(out.nbytes)
    good, above, none = np.full(sbh * sbw, 2, np.uint32), np.full(sbh * sbw, 2, np.uint32), np.zeros(sbh * sbw, np.uint32)
    above[-1] = 4

    def host(counts, max_spp=3, depth=DEPTH, scene_h=flat._h):
        return L.trhip_render_path_map(ctx._h, scene_h, C.byref(sn), None if counts is None else T._ffi.u32ptr(counts), max_spp, depth, SEED, 0, T._ffi.fptr(out), None)

    def device(counts, max_spp=3, depth=DEPTH):
        d = T._ffi.DeviceBuffer(counts.nbytes).from_host(counts)
        rc = L.trhip_render_path_map_device(ctx._h, flat._h, C.byref(sn), C.c_void_p(d.ptr), max_spp, depth, SEED, 0, C.c_void_p(d_out.ptr), None)
        d.free()
        return rc

    err = lambda: L.trhip_last_error(ctx._h)  # noqa: E731
    assert host(None, max_spp=0, depth=0) == -1 and b"null argument" in err()
    assert host(above, max_spp=0, depth=0) == -1 and b"max_spp must be" in err()
    assert host(good, max_spp=1 << 31) == -3 and b"2^32" in err()
    for call in (host, device):  # the map's refusals come before the frame's: max_depth 0 is not what is named
        assert call(above, depth=0) == -1 and b"above max_spp" in err(), call.__name__
        assert call(none, depth=0) == -1 and b"draws no sample" in err(), call.__name__
        assert call(good, depth=0) == -1 and b"max_depth" in err(), call.__name__
    prims, _ = T.scenes.cornell_primitives()
    prims[0] = T.GeometricPrimitive(prims[0].shape, None)
    bare = T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1)).flatten(ctx)
    assert host(good, scene_h=bare._h) == -3 and b"material-less" in err()
    assert not out.any()
    assert host(good) == 0 and out.any()
    d_out.free()


def records(shape, spp, seed):
    rng = np.random.default_rng(seed)
    L = rng.gamma(0.7, 1.5, (spp, *shape, 3)).astype(F)
    flat = L.reshape(spp, -1, 3)
    n = flat.shape[1]
    for k, (s, bad) in enumerate([(0, (np.nan, 1, 1)), (1, (1, np.inf, 0)), (2, (-np.inf, 0, 0)), (0, (0, 0, 0)), (1, (np.inf, -np.inf, 1)), (2, (1, 1, np.nan))]):
        flat[s % spp, (k * 11) % n] = bad
    if n > 8:
        flat[:, 7] = 0  # a black pixel
    return L


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (29, 37), (64, 64)])
def test_stats_and_map_kernels_are_their_models(T, ctx, shape):
    """Records through trhip_film_accumulate (radius 0.5: the sample bounds are the film), then the two kernels."""
    L = T.lib()
    spp = 3
    rec = records(shape, spp, 77 + shape[1])
    cam = camera(T, (shape[1], shape[0]), (0.5, 0.5))
    assert sm.sample_shape(cam)[:2] == shape
    film = np.empty((*shape, 4), F)
    sn = cam.sensor()
    ctx.check(L.trhip_film_accumulate(ctx._h, C.byref(sn), spp, SEED, 0, T._ffi.fptr(np.ascontiguousarray(rec)), T._ffi.fptr(film)))
    mv = np.empty((*shape, 2), F)
    ctx.check(L.trhip_last_sample_stats(ctx._h, T._ffi.fptr(mv)))
    ref = sm.stats_model(rec)
    assert_equal_up_to_nan_payload(mv, ref, "(m, v)")
    assert (~np.isfinite(ref)).any()
    for tau, eps, pilot, max_extra in [(0.25, 0.01, 3, 56), (1.0, 0.0, 3, 4), (np.inf, 0.01, 3, 5), (0.05, 0.5, 3, 120)]:
        p = T._ffi.SampleMapParams(tau, eps, pilot, max_extra, 0, 0)
        counts, total = np.empty(shape, np.uint32), C.c_uint64(0)
        ctx.check(L.trhip_sample_map(ctx._h, T._ffi.fptr(mv), shape[1], shape[0], C.byref(p), T._ffi.u32ptr(counts), C.byref(total)))
        ref_counts, ref_total = sm.map_model(ref, tau, eps, pilot, max_extra)
        assert np.array_equal(counts, ref_counts), (tau, int((counts != ref_counts).sum()))
        assert total.value == ref_total == int(counts.sum())
        assert np.array_equal(counts, T.api.sample_map_model(mv, tau, eps, pilot, max_extra))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("radius", [R1, WIDE])
def test_stats_on_both_record_layouts(T, ctx, fused, radius):
    L = T.lib()
    ctx.set_option("film_fused", fused)
    try:
        integ = T.PathIntegrator(camera(T, (37, 29), radius), T.SeededSampler(MAX_SPP, seed=SEED), DEPTH)
        integ.render(scene_of(T, "mesh16"))
        sbh, sbw, _, _ = sm.sample_shape(integ.camera)
        mv = np.empty((sbh, sbw, 2), F)
        ctx.check(L.trhip_last_sample_stats(ctx._h, T._ffi.fptr(mv)))
        d = T._ffi.DeviceBuffer(mv.nbytes)
        ctx.check(L.trhip_last_sample_stats_device(ctx._h, C.c_void_p(d.ptr)))
        dev = d.to_host(np.float32, mv.shape)
        d.free()
        rec = integ.sample_radiance(scene_of(T, "mesh16"))
    finally:
        ctx.set_option("film_fused", 1)
    assert_bits_equal(mv, sm.stats_model(rec), "(m, v)")
    assert_bits_equal(dev, mv, "device variant")
    assert (mv[..., 1] > 0).any()
    # a map frame's records are not a frame's: refused
    map_frame(T, "mesh16", (37, 29), radius, random_map(T, radius))
    assert L.trhip_last_sample_stats(ctx._h, T._ffi.fptr(mv)) == -1


@pytest.mark.parametrize("radius", [R1, WIDE])
def test_adaptive_integrator_is_the_public_calls_by_hand(T, ctx, radius):
    L = T.lib()
    scene, n0, max_extra, tau = scene_of(T, "cornell"), 4, MAX_SPP, 0.6
    cam = camera(T, (37, 29), radius)
    h, w = cam.film.size
    sbh, sbw, _, _ = sm.sample_shape(cam)
    ada = T.AdaptivePathIntegrator(cam, T.SeededSampler(n0, seed=SEED, sample_offset=3), DEPTH, tau=tau, max_extra=max_extra)
    film = ada.render(scene)
    # by hand
    pilot_i = T.PathIntegrator(camera(T, (37, 29), radius), T.SeededSampler(n0, seed=SEED, sample_offset=3), DEPTH)
    pilot = pilot_i.render(scene)
    rec = pilot_i.sample_radiance(scene)
    mv = np.empty((sbh, sbw, 2), F)
    ctx.check(L.trhip_last_sample_stats(ctx._h, T._ffi.fptr(mv)))
    counts, total = np.empty((sbh, sbw), np.uint32), C.c_uint64(0)
    ctx.check(L.trhip_sample_map(ctx._h, T._ffi.fptr(mv), sbw, sbh, C.byref(ada.params), T._ffi.u32ptr(counts), C.byref(total)))
    ref_counts, ref_total = sm.map_model(sm.stats_model(rec), tau, ada.params.eps, n0, max_extra)
    assert np.array_equal(counts, ref_counts) and np.array_equal(ada.counts, ref_counts) and ada.total == total.value == ref_total
    assert np.array_equal(ada.counts != 0, ref_counts != 0) and 0 < (ref_counts != 0).sum() < ref_counts.size, "the map must mix drawn and skipped pixels"
    extra_i = T.PathIntegrator(camera(T, (37, 29), radius), T.SeededSampler(n0, seed=SEED, sample_offset=3 + n0), DEPTH)
    extra = extra_i.render(scene, sample_map=T.SampleMap(counts, max_extra))
    assert_bits_equal(film[..., :3], T.Film.add(pilot, extra)[..., :3], "xyz vs trhip_film_add(pilot, extra)")
    assert_bits_equal(film[..., 3], pilot[..., 3] + extra[..., 3], "weights: the pilot's plus the map frame's")
    both = np.empty((h, w, 4), F)
    ctx.check(L.trhip_film_sum(ctx._h, T._ffi.fptr(pilot), T._ffi.fptr(extra), w, h, T._ffi.fptr(both)))
    assert_bits_equal(film, both, "film vs trhip_film_sum(pilot, extra)")
    assert ada.stats[0].camera_samples == sbh * sbw * n0 and ada.stats[1].camera_samples == ref_total
    # tau = +Inf: the pilot film, and no second frame
    inf = T.AdaptivePathIntegrator(camera(T, (37, 29), radius), T.SeededSampler(n0, seed=SEED, sample_offset=3), DEPTH, tau=np.inf, max_extra=max_extra)
    assert_bits_equal(inf.render(scene), pilot, "tau = +Inf")
    assert inf.total == 0 and inf.stats[1] is None and not inf.counts.any()
