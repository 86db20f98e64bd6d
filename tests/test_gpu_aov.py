"""First-hit feature buffers (trhip_render_aov, AOVIntegrator) on the GPU: per-sample records against the CPU oracle and the kernel-level entry points bit for bit, plane 0's
weight against the beauty frame's filter_weight_sum bit for bit, the filtered planes against a Float64 model with a derived bound, determinism, misses, refusals, the Python surface.

The record is 80 bytes (five 16-byte words), not 64: the seventeen 32-bit values the record must return bit for bit do not fit four words (tests/test_aov_api.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -23  # the bound's unit: twice the Float32 unit roundoff, so that it holds with or without FMA contraction


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(np.asarray(got, np.float32)), bits(np.asarray(ref, np.float32))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def camera(T, resolution, crop=None, radius=1.0):
    flt = T.LanczosSincFilter([radius, radius], 3.0)
    film = T.Film([resolution, resolution], T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), flt, 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def cornell_variant(T):
    """The Cornell box with a floor quad that has no material and a glass sphere whose Kt is black (base colour: Kr)."""
    prims, _ = T.scenes.cornell_primitives()
    prims[0] = T.GeometricPrimitive(prims[0].shape, None)
    prims[1] = T.GeometricPrimitive(prims[1].shape, None)
    glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(0.9, 0.8, 0.7)), T.ConstantTexture(T.RGBSpectrum(0.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)
    prims[-1] = T.GeometricPrimitive(prims[-1].shape, glass)
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


SCENES = {
    "cornell": lambda T: T.scenes.cornell_scene(),
    "shadows": lambda T: T.scenes.shadows_scene(),
    "mesh": lambda T: T.scenes.mesh_scene(16),
    "cornell_variant": cornell_variant,
}


def camera_rays(T, ob, cam, spp, seed):
    return ob.generate_rays(cam, T.scenes.camera_sample_grid(cam, spp, seed))


@pytest.mark.parametrize("which", sorted(SCENES))
def test_records_equal_the_oracle(T, ob, ctx, which):
    """t, prim and the hit geometry from orc_generate_rays + orc_trace_closest on the library's own tree; b1 / b2 from trhip_trace_closest on the same rays; material id and base
    colour from the Python scene through prim_order.  Bits, not values."""
    scene = SCENES[which](T)
    cam, spp, seed = camera(T, 48), 3, 0xA0F1
    rec = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed)).samples(scene)
    flat = scene.flatten()
    rays = camera_rays(T, ob, cam, spp, seed)
    osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
    t_ref, prim_ref, geom_ref, _ = osc.trace_closest(rays, want_geom=True)
    hit = prim_ref >= 0
    assert 0.2 < hit.mean() < 1.0, "the frame must see both hits and misses"
    rec = rec.reshape(-1)
    assert rec.size == rays.shape[0]
    assert np.array_equal(rec["prim"], prim_ref), f"{int((rec['prim'] != prim_ref).sum())} primitive ids differ"
    assert_bits_equal(rec["t"], t_ref, "t")
    assert np.isposinf(rec["t"][~hit]).all()
    assert_bits_equal(rec["p"], geom_ref[:, 0:3], "p")
    assert_bits_equal(rec["n"], geom_ref[:, 3:6], "n")
    assert_bits_equal(rec["ns"], geom_ref[:, 6:9], "ns")
    hits = flat.trace_closest(rays)
    assert_bits_equal(rec["b1"], hits["b1"], "b1")
    assert_bits_equal(rec["b2"], hits["b2"], "b2")
    order = flat.bvh()[3]
    ids, cols = T.api.primitive_materials(scene)
    caller = order[np.where(hit, prim_ref, 0)]
    assert np.array_equal(rec["material"], np.where(hit, ids[caller], -1))
    assert_bits_equal(rec["albedo"], np.where(hit[:, None], cols[caller], np.float32(0.0)), "albedo")
    if which == "cornell_variant":
        assert (rec["material"][hit] == -1).any() and not rec["albedo"][hit & (rec["material"] == -1)].any(), "a primitive without a material: id -1, base colour zero"
        glass = hit & (caller == len(ids) - 1)
        assert glass.any() and np.array_equal(rec["albedo"][glass], np.tile(np.float32([0.9, 0.8, 0.7]), (int(glass.sum()), 1))), "glass with black Kt reports Kr"
    for pad in ("pad0", "pad1", "pad2"):
        assert not rec[pad].any()
    for name in ("b1", "b2", "p", "n", "ns", "albedo"):
        assert not bits(rec[name][~hit]).any(), f"{name} must be zero on a miss"


@pytest.mark.parametrize("which", ["shadows", "mesh"])
def test_records_equal_the_kernel_level_entry_points(T, ob, ctx, which):
    scene = SCENES[which](T)
    cam, spp, seed = camera(T, 40), 2, 91
    rec = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed)).samples(scene).reshape(-1)
    flat = scene.flatten()
    samples = T.scenes.camera_sample_grid(cam, spp, seed)
    rays = np.empty((samples.shape[0], 8), np.float32)
    sn = cam.sensor()
    ctx.check(T.lib().trhip_generate_rays(ctx._h, C.byref(sn), T._ffi.fptr(samples), samples.shape[0], T._ffi.fptr(rays)))
    hits = flat.trace_closest(rays)
    geom = flat.hit_geometry(rays)
    assert (hits["prim"] >= 0).sum() > 500
    for name in ("t", "b1", "b2"):
        assert_bits_equal(rec[name], hits[name], name)
    assert np.array_equal(rec["prim"], hits["prim"])
    assert_bits_equal(rec["p"], geom[:, 0:3], "p")
    assert_bits_equal(rec["n"], geom[:, 3:6], "n")
    assert_bits_equal(rec["ns"], geom[:, 6:9], "ns")


@pytest.mark.parametrize("crop", [None, ([0.25, 0.3], [0.8, 0.9])], ids=["full", "cropped"])
def test_plane0_weight_is_the_beauty_frames(T, ctx, crop):
    scene = T.scenes.cornell_scene()
    cam, spp, seed = camera(T, 64, crop), 4, 12345
    if crop:
        assert tuple(cam.film.crop_bounds.p_min) != (1.0, 1.0)
    xyzw = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed), 1).render(scene)
    res = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed)).render(scene)
    assert res.planes.shape == (*cam.film.size, 3, 4)
    assert np.abs(xyzw[..., 3]).min() > 0
    assert_bits_equal(res.planes[..., 0, 3], xyzw[..., 3], "plane 0 weight vs filter_weight_sum")


def film_weights(T, ob, cam, samples5):
    """The Float32 weight of every (sample, film pixel) pair from the oracle's FilmTile (add_sample!, film.jl:134-164), one sample at a time into a fresh tile with the
    sample bounds of the sample's own 16 x 16 tile (integrators/sampler.jl:29-31).  Returns per sample (y0, x0, w[h, w]) in film-array coordinates."""
    sn = ob.make_sensor(cam)
    sb = cam.film.get_sample_bounds()
    sb0, sb1 = np.asarray(sb.p_min, np.float32), np.asarray(sb.p_max, np.float32)
    crop0 = np.asarray(cam.film.crop_bounds.p_min, np.float32)
    one = np.ones(3, np.float32)
    sbw, sbh = int(sb1[0] - sb0[0]) + 1, int(sb1[1] - sb0[1]) + 1
    out = []
    for i, (x, y) in enumerate(samples5[:, :2]):
        px, py = sb0[0] + (i % sbw), sb0[1] + (i // sbw) % sbh  # the sample pixel (camera_sample_grid's order), hence the tile
        t0 = np.float32([sb0[0] + 16 * ((px - sb0[0]) // 16), sb0[1] + 16 * ((py - sb0[1]) // 16)])
        tb = np.float32([t0[0], t0[1], min(t0[0] + 15, sb1[0]), min(t0[1] + 15, sb1[1])])
        bounds, size = np.empty(4, np.float32), np.empty(2, np.int32)
        h = ob.lib().orc_filmtile_new(C.byref(sn), ob.fp(tb), ob.fp(bounds), size.ctypes.data_as(C.POINTER(C.c_int32)))
        ob.lib().orc_filmtile_add_sample(h, float(x), float(y), ob.fp(one), 1.0)
        w = np.empty((int(size[0]), int(size[1]), 4), np.float32)
        ob.lib().orc_filmtile_read(h, ob.fp(w))
        ob.lib().orc_filmtile_free(h)
        out.append((int(bounds[1] - crop0[1]), int(bounds[0] - crop0[0]), w[..., 3].copy()))
    return out


def plane_model(cam, weights, rec):
    """Float64 sums of w * v over the GPU's own records, and the bound n * 2^-23 * sum |w| |v| per value (recursive summation of Float32 products, doubled: module docstring)."""
    h, w = cam.film.size
    model, mag, n = np.zeros((h, w, 3, 4)), np.zeros((h, w, 3, 4)), np.zeros((h, w))
    rec = rec.reshape(-1)
    for (y0, x0, wt), r in zip(weights, rec):
        hit = r["prim"] >= 0
        v = np.zeros((3, 4))
        v[0, 3] = 1.0
        if hit:
            v[0, :3], v[1, :3], v[1, 3], v[2, :3], v[2, 3] = r["albedo"], r["ns"], 1.0, r["p"], r["t"]
        ys, xs = slice(y0, y0 + wt.shape[0]), slice(x0, x0 + wt.shape[1])
        w64 = wt.astype(np.float64)
        model[ys, xs] += w64[..., None, None] * v
        mag[ys, xs] += np.abs(w64)[..., None, None] * np.abs(v)
        n[ys, xs] += wt != 0
    return model, n[..., None, None] * U * mag


@pytest.mark.parametrize("crop", [None, ([0.2, 0.1], [0.9, 0.7])], ids=["full", "cropped"])
def test_planes_against_a_float64_model(T, ob, ctx, crop):
    scene = T.scenes.cornell_scene()
    cam, spp, seed = camera(T, 24, crop), 3, 777
    integ = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed))
    planes = integ.render(scene).planes
    rec = integ.samples(scene)
    model, bound = plane_model(cam, film_weights(T, ob, cam, T.scenes.camera_sample_grid(cam, spp, seed)), rec)
    assert (rec["prim"] >= 0).any() and (rec["prim"] < 0).any()
    err = np.abs(planes.astype(np.float64) - model)
    print(f"planes vs Float64 model ({'cropped' if crop else 'full'}): max error / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3g}, values with a zero bound: {int((bound == 0).sum())}")
    assert err.shape == (*cam.film.size, 3, 4)
    assert np.all(err <= bound), f"{int((err > bound).sum())} of {err.size} values outside n * 2^-23 * sum|w||v|; worst {np.max(err - bound):.3g}"  # every pixel, every value


def test_determinism_sharding_and_device_variant(T, ob, ctx):
    scene = T.scenes.mesh_scene(16)
    cam, seed = camera(T, 32), 4242
    full = T.AOVIntegrator(cam, T.SeededSampler(4, seed=seed))
    a, ra = full.render(scene).planes, full.samples(scene)
    b, rb = full.render(scene).planes, full.samples(scene)
    assert_bits_equal(a, b, "planes, two calls")
    assert ra.tobytes() == rb.tobytes(), "records, two calls"
    halves = [T.AOVIntegrator(cam, T.SeededSampler(2, seed=seed, sample_offset=off)) for off in (0, 2)]
    ph = [h.render(scene).planes for h in halves]
    rh = [h.samples(scene) for h in halves]
    assert rh[0].tobytes() == ra[0:2].tobytes() and rh[1].tobytes() == ra[2:4].tobytes(), "records of the halves are the slices of the whole"
    _, bound = plane_model(cam, film_weights(T, ob, cam, T.scenes.camera_sample_grid(cam, 4, seed)), ra)
    err = np.abs(a.astype(np.float64) - (ph[0].astype(np.float64) + ph[1].astype(np.float64)))
    assert np.all(err <= bound), f"{int((err > bound).sum())} values of spp 4 differ from the sum of two spp-2 shards by more than the bound"
    # the _device variant: both outputs to device memory
    h, w = cam.film.size
    d_planes, d_rec = T._ffi.DeviceBuffer(h * w * 12 * 4), T._ffi.DeviceBuffer(ra.size * 80)
    sn, st, flat = cam.sensor(), T.Stats(), scene.flatten()
    ctx.check(T.lib().trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), 4, seed, 0, C.c_void_p(d_planes.ptr), C.c_void_p(d_rec.ptr), C.byref(st)))
    assert_bits_equal(d_planes.to_host(np.float32, (h, w, 3, 4)), a, "planes, device variant")
    assert d_rec.to_host(T._ffi.AOV_DTYPE, ra.shape).tobytes() == ra.tobytes(), "records, device variant"
    assert st.camera_samples == ra.size == st.closest_rays and st.shadow_rays == 0 and st.launches_raygen == 1 and st.launches_shade == 1 and st.launches_film == 1
    path = T.PathIntegrator(cam, T.SeededSampler(4, seed=seed), 1)
    path.render(scene)
    assert st.traversal == path.stats.traversal and st.fallback_rays <= st.closest_rays and st.ms_total > 0
    full.render(scene, device_out=d_planes.zero().ptr)
    assert_bits_equal(d_planes.to_host(np.float32, (h, w, 3, 4)), a, "planes, AOVIntegrator.render(device_out=)")
    d_planes.free()
    d_rec.free()


def test_misses_and_refusals(T, ctx):
    scene = T.scenes.cornell_scene()
    flt = T.LanczosSincFilter([1.0, 1.0], 3.0)
    film = T.Film([32, 32], T.Bounds2([0.0, 0.0], [1.0, 1.0]), flt, 1.0, 1.0, "")
    away = T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 30, 102], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)
    integ = T.AOVIntegrator(away, T.SeededSampler(2, seed=5))
    rec, res = integ.samples(scene), integ.render(scene)
    assert np.isposinf(rec["t"]).all() and (rec["prim"] == -1).all() and (rec["material"] == -1).all()
    for name in ("b1", "b2", "p", "n", "ns", "albedo", "pad0", "pad1", "pad2"):
        assert not bits(rec[name]).any(), name
    xyzw = T.PathIntegrator(away, T.SeededSampler(2, seed=5), 1).render(scene)
    assert_bits_equal(res.planes[..., 0, 3], xyzw[..., 3], "plane 0 weight of an all-miss frame")
    assert not bits(res.planes[..., 0, :3]).any() and not bits(res.planes[..., 1:, :]).any()
    assert not res.alpha.any() and not res.depth.any()
    # refusals
    flat, sn, st = scene.flatten(), away.sensor(), T.Stats()
    assert T.lib().trhip_render_aov(ctx._h, flat._h, C.byref(sn), 2, 5, 0, None, None, C.byref(st)) == -1  # TRHIP_ERR_INVALID
    assert T.lib().trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), 2, 5, 0, None, None, C.byref(st)) == -1
    raw = C.c_void_p()
    ctx.check(T.lib().trhip_scene_new(ctx._h, C.byref(raw)))
    try:
        out = np.empty((32, 32, 3, 4), np.float32)
        assert T.lib().trhip_render_aov(ctx._h, raw, C.byref(sn), 2, 5, 0, T._ffi.fptr(out), None, C.byref(st)) == -1
        assert b"not committed" in T.lib().trhip_last_error(ctx._h)
    finally:
        T.lib().trhip_scene_free(raw)
    # a scene without lights and with a material-less primitive renders
    prims, _ = T.scenes.cornell_primitives()
    prims[2] = T.GeometricPrimitive(prims[2].shape, None)
    dark = T.Scene([], T.BVHAccel(prims, 1))
    assert (T.AOVIntegrator(camera(T, 16), T.SeededSampler(1, seed=1)).samples(dark)["prim"] >= 0).any()


@pytest.mark.parametrize("radius", [1.0, 0.5])
def test_python_surface(T, ctx, radius):
    scene = T.scenes.cornell_scene()
    cam = camera(T, 48, radius=radius)
    assert np.asarray(cam.film.filter_table).min() >= 0, "the alpha bounds below need a filter without negative weights"
    integ = T.AOVIntegrator(cam, T.SeededSampler(4, seed=31))
    res = integ.render(scene)
    h, w = cam.film.size
    assert res.planes.shape == (h, w, 3, 4) and res.albedo.shape == res.normal.shape == res.position.shape == (h, w, 3) and res.depth.shape == res.alpha.shape == (h, w)
    rec = integ.samples(scene)
    sb = cam.film.get_sample_bounds()
    assert rec.shape == (4, int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1) and rec.dtype == T._ffi.AOV_DTYPE
    # coverage of a film pixel from the records: a pixel is reached only by sample pixels within ceil(radius + 0.5) + 1 of it
    hit = (rec["prim"] >= 0)
    reach = int(np.ceil(radius + 0.5)) + 1
    off = int(cam.film.crop_bounds.p_min[0] - sb.p_min[0]) + reach
    pad = ((0, 0), (reach, reach), (reach, reach))
    hit_or_absent, hit_and_present = np.pad(hit, pad, constant_values=True), np.pad(hit, pad, constant_values=False)  # sample pixels outside the sample bounds do not exist
    full = np.ones((h, w), bool)
    none = np.ones((h, w), bool)
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            full &= hit_or_absent[:, off + dy:off + dy + h, off + dx:off + dx + w].all(axis=0)
            none &= ~hit_and_present[:, off + dy:off + dy + h, off + dx:off + dx + w].any(axis=0)
    assert full.sum() > 100 and (~full).sum() > 100
    assert np.all(res.alpha[full] == 1.0), "alpha is 1 where every sample in reach hits"
    assert np.all(res.alpha[none] == 0.0)
    assert np.all((res.alpha >= 0.0) & (res.alpha <= 1.0))
    mixed = ~full & ~none
    assert ((res.alpha[mixed] > 0) & (res.alpha[mixed] < 1)).any()
    # non-negative weights: a covered pixel's normal is a convex combination of unit normals, its depth one of positive depths
    assert np.all(res.depth[full] > 0) and np.all(np.linalg.norm(res.normal[full], axis=-1) <= 1.0 + 1e-5)
    st = integ.stats
    assert st.camera_samples == rec.size and st.closest_rays == rec.size
