"""GPU parity tests (run with -m gpu on an MI355X): every stage of the hot path, through the C ABI, against the CPU
oracle on the same seeded inputs.  Bar: BIT-EXACT (Float32 bit patterns) — the kernels share the oracle's operation
order, the deterministic elementary functions and the counter-based sampler, and are built without FMA contraction.
"""
import numpy as np
import pytest
from conftest import experiments

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[pytest.param(4, marks=experiments("traversal", 4)), pytest.param(6, marks=experiments("traversal", 6)), pytest.param(7, marks=experiments("traversal", 7)), 2, 3, 1],
                ids=["trace8", "trace4x2", "trace7", "trace2", "trace3", "trace1"])
def traversal(request, ctx):
    """Every parity test runs with all traversal kernels: 4 = k_trace8 (8-wide quantised nodes in the binary walk's order; the
    default), 2 = k_trace2 (children-in-parent nodes, per-lane ray replacement), 3 = k_trace3 (the same with leaves postponed
    and tested together), 1 = the literal accel/bvh.jl loop."""
    ctx.set_option("traversal", request.param)
    ctx.set_option("compose_spheres", 1)  # scenes of this module are committed with their spheres as a chain, so that 4 really runs k_trace8
    yield request.param
    ctx.set_option("traversal", 3)
    ctx.set_option("compose_spheres", -1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    # NaN payloads may differ between producers; compare NaN-ness there and bits elsewhere
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN pattern differs"
    bad = (bits(a) != bits(b)) & ~na
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} values differ, first at {np.argwhere(bad)[0]}: {a[tuple(np.argwhere(bad)[0])]!r} vs {b[tuple(np.argwhere(bad)[0])]!r}"


def scene_pair(T, ob, scene):
    flat = scene.flatten()
    osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
    return flat, osc


def camera_rays(T, ob, cam, spp=1, seed=3):
    samples = T.scenes.camera_sample_grid(cam, spp, seed)
    return ob.generate_rays(cam, samples)


@pytest.fixture(scope="module")
def shadows(T, ob, ctx):
    scene = T.scenes.shadows_scene()
    ctx.set_option("tiny_scene_prims", 0)  # keep the hierarchy: the single-leaf form has its own test below
    try:
        flat, osc = scene_pair(T, ob, scene)
    finally:
        ctx.set_option("tiny_scene_prims", 16)
    assert flat.bvh()[1].size > 1
    return scene, flat, osc


@pytest.fixture(scope="module")
def mesh(T, ob, ctx):
    scene = T.scenes.mesh_scene(64)  # 8 192 triangles + Cornell box + 2 spheres
    flat, osc = scene_pair(T, ob, scene)
    return scene, flat, osc


def test_generate_rays_matches_oracle(T, ob, ctx):
    """a3: generate_ray (camera/perspective.jl:85-114) incl. the thin-lens branch."""
    import ctypes as C
    for lens_radius in (0.0, 0.05):
        cam = T.scenes.shadows_camera(48)
        cam.lens_radius = np.float32(lens_radius)
        cam.focal_distance = np.float32(52.0)
        samples = T.scenes.camera_sample_grid(cam, 2, seed=11)
        ref = ob.generate_rays(cam, samples)
        out = np.empty_like(ref)
        sn = cam.sensor()
        ctx.check(T.lib().trhip_generate_rays(ctx._h, C.byref(sn), T._ffi.fptr(samples), samples.shape[0], T._ffi.fptr(out)))
        assert_bits_equal(out, ref, f"generate_ray lens_radius={lens_radius}")


def test_tiny_scene_is_one_leaf(T, ob, ctx):
    """Scenes of <= 16 primitives are committed as a single leaf (th_bvh.h): same hits as the oracle walking that leaf,
    closest and any-hit, camera and incoherent rays."""
    scene = T.scenes.shadows_scene()
    flat, osc = scene_pair(T, ob, scene)
    bounds, a, flags, order = flat.bvh()
    assert a.size == 1 and (flags[0] & 3) == 3 and (flags[0] >> 2) == order.size == flat.n_prims
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, T.scenes.shadows_camera(64)), T.scenes.incoherent_rays(30000, wb[:3] - 0.2, wb[3:] + 0.2)])
    got = flat.trace_closest(rays)
    t_ref, prim_ref, _, _ = osc.trace_closest(rays)
    assert (prim_ref >= 0).sum() > 1000
    assert np.array_equal(got["prim"], prim_ref)
    assert_bits_equal(got["t"], t_ref, "t (single leaf)")
    assert np.array_equal(flat.trace_any(rays), osc.trace_any(rays)[0])


@pytest.mark.parametrize("which", ["shadows", "mesh"])
def test_trace_closest_camera_and_incoherent(T, ob, which, shadows, mesh):
    """a6-a9: closest-hit traversal + Triangle/Sphere intersection: t and primitive bit-exact on the same BVH."""
    scene, flat, osc = shadows if which == "shadows" else mesh
    cam = T.scenes.shadows_camera(96)
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, cam), T.scenes.incoherent_rays(60000, wb[:3] - 0.2, wb[3:] + 0.2)])
    hits = flat.trace_closest(rays)
    t_ref, prim_ref, _, _ = osc.trace_closest(rays)
    assert (prim_ref >= 0).sum() > 1000
    assert np.array_equal(hits["prim"], prim_ref), f"{int((hits['prim'] != prim_ref).sum())} primitive ids differ"
    assert_bits_equal(hits["t"], t_ref, "t_hit")


@pytest.mark.parametrize("which", ["shadows", "mesh"])
def test_trace_any(T, ob, which, shadows, mesh):
    """a6: intersect_p (accel/bvh.jl:260-299), including finite t_max and unnormalised directions (shadow rays, A.8)."""
    scene, flat, osc = shadows if which == "shadows" else mesh
    wb = osc.world_bound()
    rays = T.scenes.incoherent_rays(50000, wb[:3] - 0.2, wb[3:] + 0.2, seed=99)
    rays[::3, 4:7] *= 3.7     # unnormalised
    rays[::5, 3] = 0.4        # finite t_max
    occ = flat.trace_any(rays)
    occ_ref, _ = osc.trace_any(rays)
    assert 0.05 < occ_ref.mean() < 0.999
    assert np.array_equal(occ, occ_ref)


@pytest.mark.parametrize("which", ["shadows", "mesh"])
def test_hit_geometry(T, ob, which, shadows, mesh):
    """a8-a11: the SurfaceInteraction / BSDF frame the shading kernel rebuilds: p, n, ns, wo, ss bit-exact."""
    scene, flat, osc = shadows if which == "shadows" else mesh
    cam = T.scenes.shadows_camera(64)
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, cam, seed=5), T.scenes.incoherent_rays(20000, wb[:3], wb[3:], seed=6)])
    geom = flat.hit_geometry(rays)
    _, prim_ref, geom_ref, _ = osc.trace_closest(rays, want_geom=True)
    assert (prim_ref >= 0).sum() > 500
    assert_bits_equal(geom, geom_ref, "hit geometry (p n ns wo ss)")


def _frames(n, seed):
    rng = np.random.default_rng(seed)
    ns = rng.normal(size=(n, 3)).astype(np.float32)
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    ng = ns + 0.05 * rng.normal(size=(n, 3)).astype(np.float32)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    t = np.cross(ns, rng.normal(size=(n, 3))).astype(np.float32)
    return np.concatenate([ng, ns, t], axis=1).astype(np.float32)


def _dirs(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


MATERIALS = {
    "matte": lambda T: T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.8, 0.5, 0.3)), T.ConstantTexture(0.0)),
    "oren_nayar": lambda T: T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.8, 0.5, 0.3)), T.ConstantTexture(25.0)),
    "mirror": lambda T: T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.9))),
    "glass": lambda T: T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(T.RGBSpectrum(0.9, 1.0, 0.8)), T.ConstantTexture(0.0), T.ConstantTexture(0.0),
                                       T.ConstantTexture(1.5), True),
    "rough_glass": lambda T: T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(0.3), T.ConstantTexture(0.2),
                                             T.ConstantTexture(1.33), True),
    "plastic": lambda T: T.PlasticMaterial(T.ConstantTexture(T.RGBSpectrum(0.64)), T.ConstantTexture(T.RGBSpectrum(0.1)), T.ConstantTexture(0.010408001), True),
    "plastic_noremap": lambda T: T.PlasticMaterial(T.ConstantTexture(T.RGBSpectrum(0.3, 0.6, 0.2)), T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.15), False),
}


@pytest.mark.parametrize("name", list(MATERIALS))
@pytest.mark.parametrize("multi", [False, True])
def test_bsdf_eval_and_sample(T, ob, ctx, name, multi):
    """a10, a12, a13: materials -> lobes, BSDF f / pdf / sample_f for every BxDF the materials can add."""
    mat = MATERIALS[name](T)
    tri = T.create_triangle_mesh(T.ShapeCore(T.translate([0, 0, 0]), False), 1, np.array([1, 2, 3], np.uint32), 3, [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    scene = T.Scene([], T.BVHAccel([T.GeometricPrimitive(tri[0], mat)], 1))
    flat, osc = scene_pair(T, ob, scene)
    n = 20000
    frames = _frames(n, 1)
    wo, wi = _dirs(n, 2), _dirs(n, 3)
    rng = np.random.default_rng(4)
    u = rng.random((n, 2), dtype=np.float32)
    ALL = 31
    for flags in (ALL, ALL & ~16, 1 | 16, 2 | 16):
        d0 = np.concatenate([wo, wi], axis=1)
        assert_bits_equal(flat.bsdf_query(0, multi, 0, flags, frames, d0), osc.bsdf_query(0, multi, 0, flags, frames, d0), f"{name} f/pdf flags={flags}")
        d1 = np.concatenate([wo, u, np.zeros((n, 1), np.float32)], axis=1)
        assert_bits_equal(flat.bsdf_query(0, multi, 1, flags, frames, d1), osc.bsdf_query(0, multi, 1, flags, frames, d1), f"{name} sample_f flags={flags}")


@pytest.mark.parametrize("res,spp,depth", [(40, 3, 5), (64, 2, 8)])
def test_render_path_shadows_bit_exact(T, ob, shadows, res, spp, depth):
    """a1-a16 end to end on config C1's scene: per-sample radiance AND film accumulators bit-exact."""
    scene, flat, osc = shadows
    cam = T.scenes.shadows_camera(res)
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=0x5EED0001), depth)
    xyzw = integ.render(scene)
    L = integ.sample_radiance(scene)
    ref_xyzw, ref_L, st = osc.render(cam, "path", spp, depth, seed=0x5EED0001, want_samples=True)
    assert ref_L.max() > 0
    assert_bits_equal(L, ref_L, "per-sample radiance")
    assert_bits_equal(xyzw, ref_xyzw, "film xyz + weight sums")
    assert integ.stats.camera_samples == st.camera_samples
    assert integ.stats.closest_rays == st.closest_rays
    assert integ.stats.shadow_rays == st.shadow_rays


def test_render_path_mesh_bit_exact(T, ob, mesh):
    scene, flat, osc = mesh
    cam = T.scenes.cornell_camera(48)
    integ = T.PathIntegrator(cam, T.SeededSampler(2, seed=42), 6)
    xyzw = integ.render(scene)
    L = integ.sample_radiance(scene)
    ref_xyzw, ref_L, st = osc.render(cam, "path", 2, 6, seed=42, want_samples=True)
    assert_bits_equal(L, ref_L, "per-sample radiance")
    assert_bits_equal(xyzw, ref_xyzw, "film")
    assert integ.stats.closest_rays == st.closest_rays and integ.stats.shadow_rays == st.shadow_rays


def test_render_batches_and_sample_offset(T, ob, ctx, shadows):
    """Batching must not change results; sample_offset shifts the sampler streams (multi-GPU sharding, §8e)."""
    scene, flat, osc = shadows
    cam = T.scenes.shadows_camera(32)
    a = T.PathIntegrator(cam, T.SeededSampler(4, seed=9), 4).render(scene).copy()
    ctx.set_option("batch_paths", 34 * 34 + 5)  # one sample pass per batch
    try:
        b = T.PathIntegrator(cam, T.SeededSampler(4, seed=9), 4).render(scene).copy()
    finally:
        ctx.set_option("batch_paths", 0)
    assert_bits_equal(a, b, "batched film")
    for overlap in (0, 1):  # single-stream schedule / shadow rays on a second stream (the default is the second stream since round 5)
        ctx.set_option("overlap", overlap)
        try:
            c = T.PathIntegrator(cam, T.SeededSampler(4, seed=9), 4).render(scene).copy()
        finally:
            ctx.set_option("overlap", 1)
        assert_bits_equal(a, c, f"film with overlap = {overlap}")
    ctx.set_option("pipelines", 4)  # four batches in flight on separate stream pairs
    ctx.set_option("batch_paths", 4 * 34 * 34)
    try:
        d = T.PathIntegrator(cam, T.SeededSampler(4, seed=9), 4).render(scene).copy()
    finally:
        ctx.set_option("pipelines", 1)
        ctx.set_option("batch_paths", 0)
    assert_bits_equal(a, d, "film with concurrent pipelines")
    # two half renders with offsets sum (in fp32, tolerance) to the full one
    h0 = T.PathIntegrator(cam, T.SeededSampler(2, seed=9, sample_offset=0), 4).render(scene).copy()
    h1 = T.PathIntegrator(cam, T.SeededSampler(2, seed=9, sample_offset=2), 4).render(scene).copy()
    np.testing.assert_allclose(h0 + h1, a, rtol=2e-5, atol=1e-6)
    ref, _, _ = osc.render(cam, "path", 2, 4, seed=9, sample_offset=2)
    assert_bits_equal(h1, ref, "offset film")


def test_film_accumulate_matches_oracle_tile_order(T, ob, ctx):
    """a16: add_sample! + merge_film_tile! for arbitrary radiance incl. NaN samples (integrators/sampler.jl:46) and a wide filter."""
    import ctypes as C
    flt = T.LanczosSincFilter([2.5, 1.5], 3.0)
    film = T.Film([37, 29], T.Bounds2([0.0, 0.0], [1.0, 1.0]), flt, 1.0, 1.0, "")
    cam = T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)
    # a scene with nothing in it: the oracle render then only exercises the film; feed radiance through a constant trick:
    # use the real path instead — render the shadows scene and compare the film of GPU accumulate fed with the ORACLE's samples
    scene = T.scenes.shadows_scene()
    osc = ob.OracleScene.from_scene(scene)
    spp = 3
    ref_xyzw, ref_L, _ = osc.render(cam, "path", spp, 3, seed=5, want_samples=True)
    sn = cam.sensor()
    out = np.empty_like(ref_xyzw)
    ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, 5, 0, T._ffi.fptr(ref_L), T._ffi.fptr(out)))
    assert_bits_equal(out, ref_xyzw, "film accumulate (wide anisotropic filter)")  # too wide for the packed descriptor: the 1 x 4 block gather, on an odd film size


def test_film_gather_from_packed_descriptors(T, ob, ctx):
    """The default film pass for filter radii <= 1 (every scene of the reference): the sample's pixel range and filter-table indices ride as 30 bits in the
    .w lane of its radiance record and a thread owns 2 x 4 film pixels (k_film_gather_packed).  Records re-laid pixel-group-major (k_film_pack_transpose) and
    in place (k_film_pack_w, film_relayout 0), odd film sizes, a crop window, radii 1, 0.5 and anisotropic — against the oracle's add_sample! / merge_film_tile!
    loop; NaN samples against the film the oracle's film-tile calls make of the records after the NaN rule (sample_map_model.film_model)."""
    import ctypes as C
    import sample_map_model as sm
    scene = T.scenes.shadows_scene()
    osc = ob.OracleScene.from_scene(scene)
    for res, crop, radius, spp in (([37, 29], ([0.0, 0.0], [1.0, 1.0]), [1.0, 1.0], 3), ([64, 48], ([0.0, 0.0], [1.0, 1.0]), [1.0, 1.0], 5), ([53, 41], ([0.2, 0.1], [0.9, 0.8]), [1.0, 0.5], 2),
                                   ([33, 70], ([0.0, 0.0], [1.0, 1.0]), [0.6, 0.95], 4)):
        flt = T.LanczosSincFilter(radius, 3.0)
        film = T.Film(res, T.Bounds2(crop[0], crop[1]), flt, 1.0, 1.0, "")
        cam = T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)
        ref_xyzw, ref_L, _ = osc.render(cam, "path", spp, 3, seed=5, want_samples=True)
        sn = cam.sensor()
        # NaN samples are zeroed (integrators/sampler.jl:46): a record that holds a NaN counts as (0, 0, 0), its filter weight still counts
        bad_L = ref_L.copy()
        bad_L.reshape(-1, 3)[::97, 1] = np.nan
        ruled = bad_L.reshape(-1, 3).copy()
        ruled[np.isnan(ruled).any(axis=1)] = 0.0
        sbh, sbw, _, _ = sm.sample_shape(cam)
        ref_nan = sm.film_model(ob, cam, ruled.reshape(spp, sbh, sbw, 3), np.full((sbh, sbw), spp), 5)
        for relayout in (1, 0):  # 0: descriptors written in place, sample-major gather
            ctx.set_option("film_relayout", relayout)
            try:
                out, out_nan = np.empty_like(ref_xyzw), np.empty_like(ref_xyzw)
                ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, 5, 0, T._ffi.fptr(ref_L), T._ffi.fptr(out)))
                ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, 5, 0, T._ffi.fptr(bad_L), T._ffi.fptr(out_nan)))
            finally:
                ctx.set_option("film_relayout", 1)
            assert_bits_equal(out, ref_xyzw, f"film {res}, radius {radius}, relayout={relayout}")
            assert_bits_equal(out_nan, ref_nan, f"NaN samples, film {res}, radius {radius}, relayout={relayout}")


def test_film_to_rgb(T, ob, ctx, shadows):
    scene, flat, osc = shadows
    cam = T.scenes.shadows_camera(32)
    T.PathIntegrator(cam, T.SeededSampler(2, seed=1), 3).render(scene)
    rgb = cam.film.to_rgb()
    h, w = cam.film.size
    xyzw = np.concatenate([cam.film.xyz, cam.film.filter_weight_sum[..., None]], axis=-1).astype(np.float32)
    ref = np.empty((h, w, 3), np.float32)
    ob.lib().orc_film_to_rgb(ob.fp(np.ascontiguousarray(xyzw)), w, h, 1.0, ob.fp(ref))
    assert_bits_equal(rgb, ref, "film_to_rgb")


def test_partial_spheres_and_transforms(T, ob, ctx):
    """a9: clipped spheres (z_min / z_max / ϕ_max, sphere.jl:13-26, 65-69), reversed orientation and a scaled
    (non-rigid) object_to_world — the slow clipping path next to the full-sphere fast path."""
    mat = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.7)), T.ConstantTexture(0.0))
    glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)
    prims = [
        T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.25, 0.3, -2.5]), False), 0.2, -0.1, 0.15, 250.0), mat),
        T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.7, 0.3, -2.6]), True), 0.25, -0.25, 0.1, 360.0), glass),
        T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.5, 0.7, -2.4]) * T.scale(1.0, 0.5, 1.5), False), 0.2, 360.0), mat),
        T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.5, 0.15, -2.2]), False), 0.12, 359.0), mat),
    ]
    floor = T.create_triangle_mesh(T.ShapeCore(T.translate([0, 0, -3]), True), 2, np.array([1, 2, 3, 1, 3, 4], np.uint32), 4, [[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]])
    prims += [T.GeometricPrimitive(t, mat) for t in floor]
    scene = T.Scene([T.PointLight(T.translate([0.5, 0.95, -2.1]), T.RGBSpectrum(3.0)), T.SpotLight(T.translate([0.1, 0.9, -2.0]), T.RGBSpectrum(4.0), 50.0, 30.0)], T.BVHAccel(prims, 1))
    flat, osc = scene_pair(T, ob, scene)
    cam = T.scenes.shadows_camera(64)
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, cam, seed=21), T.scenes.incoherent_rays(40000, wb[:3] - 0.1, wb[3:] + 0.1, seed=22)])
    hits = flat.trace_closest(rays)
    t_ref, prim_ref, geom_ref, _ = osc.trace_closest(rays, want_geom=True)
    assert len(set(prim_ref[prim_ref >= 0])) == 6
    assert np.array_equal(hits["prim"], prim_ref)
    assert_bits_equal(hits["t"], t_ref, "t_hit")
    assert_bits_equal(flat.hit_geometry(rays), geom_ref, "geometry")
    occ_ref, _ = osc.trace_any(rays)
    assert np.array_equal(flat.trace_any(rays), occ_ref)
    integ = T.PathIntegrator(cam, T.SeededSampler(2, seed=77), 5)
    xyzw = integ.render(scene)
    ref_xyzw, ref_L, _ = osc.render(cam, "path", 2, 5, seed=77, want_samples=True)
    assert_bits_equal(integ.sample_radiance(scene), ref_L, "per-sample radiance (two lights, spot falloff)")
    assert_bits_equal(xyzw, ref_xyzw, "film")
    # the same primitives under a hierarchy (k_trace3 / k_trace2 built WITH the clipped-sphere code) instead of one leaf (k_trace_leaf)
    ctx.set_option("tiny_scene_prims", 0)
    try:
        scene2 = T.Scene(scene.lights, T.BVHAccel(prims, 1))
        flat2 = scene2.flatten(ctx)
        assert flat2.bvh()[1].size > 1
        osc2 = ob.OracleScene.from_scene(scene2, bvh=flat2.bvh())
        t2, prim2, _, _ = osc2.trace_closest(rays)
        occ2, _ = osc2.trace_any(rays)
        from conftest import supported
        for trav in supported(ctx, "traversal", (7, 6, 4, 3, 2, 1)):
            ctx.set_option("traversal", trav)
            h2 = flat2.trace_closest(rays)
            assert np.array_equal(h2["prim"], prim2), trav
            assert_bits_equal(h2["t"], t2, f"t_hit (hierarchy, traversal {trav})")
            assert np.array_equal(flat2.trace_any(rays), occ2), trav
    finally:
        ctx.set_option("tiny_scene_prims", 16)
        ctx.set_option("traversal", 3)


def test_streaming_wavefront_matches_classic_and_oracle(T, ob, ctx, traversal):
    """PathIntegrator as a streaming wavefront (th_trace2.h): rays over the fetch budget are suspended with their traversal
    stack and resumed in the next round; per-depth radiance terms are folded in order.  Film and per-sample radiance must
    equal the classic per-depth wavefront and the oracle bit for bit, whatever the budget (1 = every ray is cut at every
    interior node) and the list capacity (a full list makes rays run to their end in place)."""
    if traversal == 1:
        pytest.skip("streaming is built on k_trace2")
    scene = T.scenes.mesh_scene(24)
    cam = T.scenes.cornell_camera(32)
    flat = scene.flatten(ctx)
    osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
    ref, ref_L, _ = osc.render(cam, "path", 4, 6, seed=21, want_samples=True)

    def render(**opts):
        for k, v in opts.items():
            ctx.set_option(k, v)
        try:
            integ = T.PathIntegrator(cam, T.SeededSampler(4, seed=21), 6)
            film = integ.render(scene, ctx).copy()
            return film, integ.sample_radiance(scene).copy(), integ.stats
        finally:
            ctx.set_option("streaming", 0)
            ctx.set_option("stream_budget_min", 2048)
            ctx.set_option("stream_list_cap", 0)
            ctx.set_option("overlap", 1)

    classic, classic_L, st0 = render(streaming=0)
    assert_bits_equal(classic, ref, "classic film")
    for opts in ({"streaming": 0, "overlap": 1}, {"streaming": 0, "overlap": 0}, {"streaming": 1}, {"streaming": 1, "stream_budget_min": 1}, {"streaming": 1, "stream_budget_min": 7}, {"streaming": 1, "stream_budget_min": 3, "stream_list_cap": 64},
                 {"streaming": 1, "stream_budget_min": 2, "overlap": 0}):
        film, L, st = render(**opts)
        assert_bits_equal(L, classic_L, f"per-sample radiance, {opts}")
        assert_bits_equal(film, ref, f"film, {opts}")
        assert st.closest_rays == st0.closest_rays and st.shadow_rays == st0.shadow_rays, opts
    # streaming + the two-stream mode on a FRESH context (no classic frame has sized the poison notes of the two-stream classic path: the
    # streaming path must not read them), and again after a classic two-stream frame left stale notes behind
    fresh = T.Context(0)
    try:
        fresh.set_option("traversal", traversal)
        fresh.set_option("compose_spheres", 1)  # the same tree as `ctx` built (the module's fixture): another tree resolves equal-t ties differently
        scene.flatten(fresh)
        for pre_classic in (False, True):
            if pre_classic:
                fresh.set_option("overlap", 1)
                T.PathIntegrator(T.scenes.cornell_camera(40), T.SeededSampler(2, seed=5), 3).render(scene, fresh)
            for opts in ({"streaming": 1, "overlap": 1}, {"streaming": 1, "overlap": 1, "stream_budget_min": 2}):
                for k, v in opts.items():
                    fresh.set_option(k, v)
                integ = T.PathIntegrator(cam, T.SeededSampler(4, seed=21), 6)
                film = integ.render(scene, fresh).copy()
                assert_bits_equal(integ.sample_radiance(scene), classic_L, f"per-sample radiance, fresh context, {opts}")
                assert_bits_equal(film, ref, f"film, fresh context, {opts}")
                fresh.set_option("streaming", 0)
                fresh.set_option("stream_budget_min", 2048)
    finally:
        if scene._flat is not None and scene._flat.ctx is fresh:  # the scene's device copy on the context about to go
            scene._flat.free()
            scene._flat = None
        fresh.close()


def test_render_closed_mesh_scene(T, ob, ctx):
    """S-blob (a closed displaced cube-sphere in the Cornell walls; triangle primitives directly followed by a mesh group in the
    scene list): film and per-sample radiance bit-exact."""
    scene = T.scenes.blob_scene(10)
    cam = T.scenes.cornell_camera(28)
    flat = scene.flatten(ctx)
    assert flat.bvh()[3].size == 10 + 12 * 10 * 10
    osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
    ref, ref_L, _ = osc.render(cam, "path", 3, 5, seed=77, want_samples=True)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=77), 5)
    film = integ.render(scene, ctx)
    assert_bits_equal(integ.sample_radiance(scene), ref_L, "per-sample radiance (S-blob)")
    assert_bits_equal(film, ref, "film (S-blob)")


@experiments("bvh_builder", 1)
def test_device_built_lbvh(T, ob, ctx):
    """BVHAccel built on the device (th_lbvh.h, option bvh_builder = 1): a valid BVH2 in the reference's flat layout — every
    primitive in exactly one leaf, first child = i + 1, child boxes inside their parent's, leaf boxes = primitive bounds — and
    the same hits / film as the oracle walking that tree."""
    ctx.set_option("bvh_builder", 1)
    try:
        scene = T.scenes.mesh_scene(40)  # 3 200 triangles + Cornell box + 2 spheres
        flat = scene.flatten(ctx)
    finally:
        ctx.set_option("bvh_builder", -1)
    bounds, a, flags, order = flat.bvh()
    n = order.size
    assert a.size == 2 * n - 1 and sorted(order.tolist()) == list(range(n))
    leaf = (flags & 3) == 3
    assert leaf.sum() == n and np.all(flags[leaf] >> 2 == 1) and sorted(a[leaf].tolist()) == list(range(n))
    inner = np.flatnonzero(~leaf)
    assert np.all(a[inner] > inner + 1) and np.all(a[inner] < a.size) and np.all(flags[inner] <= 2)
    for child in (inner + 1, a[inner]):  # both children lie inside the parent box
        assert np.all(bounds[child, :3] >= bounds[inner, :3]) and np.all(bounds[child, 3:] <= bounds[inner, 3:])
    # subtree sizes: the second child starts right after the first child's subtree, the root spans everything
    size = np.ones(a.size, np.int64)
    for i in inner[::-1]:
        size[i] = 1 + size[i + 1] + size[a[i]]
        assert a[i] == i + 1 + size[i + 1]
    assert size[0] == a.size
    osc = ob.OracleScene.from_scene(scene, bvh=(bounds, a, flags, order))
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, T.scenes.cornell_camera(64)), T.scenes.incoherent_rays(40000, wb[:3] - 0.2, wb[3:] + 0.2)])
    got = flat.trace_closest(rays)
    t_ref, prim_ref, _, _ = osc.trace_closest(rays)
    assert np.array_equal(got["prim"], prim_ref)
    assert_bits_equal(got["t"], t_ref, "t (device-built BVH)")
    assert np.array_equal(flat.trace_any(rays), osc.trace_any(rays)[0])
    cam = T.scenes.cornell_camera(24)
    ref, _, _ = osc.render(cam, "path", 2, 5, seed=4)
    assert_bits_equal(T.PathIntegrator(cam, T.SeededSampler(2, seed=4), 5).render(scene, ctx), ref, "film (device-built BVH)")


def test_film_records_written_by_raygen_equal_the_pack_pass(T, ob, ctx):
    """Option film_fused (default on): k_raygen writes the radiance records in the gather's layout with their splat descriptors.  Film and per-sample
    radiance must not depend on it — whole frames, banded frames (band_tile_rows), several sample passes per frame (batch_paths)."""
    scene = T.scenes.cornell_scene()
    cam = T.scenes.cornell_camera(40)
    osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten(ctx).bvh())
    ref, ref_L, _ = osc.render(cam, "path", 5, 4, seed=123, want_samples=True)
    try:
        for opts in ({}, {"band_tile_rows": 1}, {"batch_paths": 42 * 42 * 2}):
            for fused in (1, 0):
                ctx.set_option("film_fused", fused)
                for k, v in opts.items():
                    ctx.set_option(k, v)
                integ = T.PathIntegrator(cam, T.SeededSampler(5, seed=123), 4)
                film = integ.render(scene, ctx)
                assert_bits_equal(film, ref, f"film (film_fused {fused}, {opts})")
                if "band_tile_rows" not in opts:  # per-sample radiance is kept for whole frames only
                    assert_bits_equal(integ.sample_radiance(scene), ref_L, f"per-sample radiance (film_fused {fused}, {opts})")
                for k in opts:
                    ctx.set_option(k, 0)
    finally:
        ctx.set_option("film_fused", 1)
        ctx.set_option("band_tile_rows", 0)
        ctx.set_option("batch_paths", 0)


@experiments("leaf_sorted", 1)
def test_one_leaf_scene_sorted_by_candidates(T, ob, ctx):
    """Option leaf_sorted (th_leaf2.h; off by default — measured slower): a one-leaf scene's rays grouped by the primitives they can hit before the leaf is walked.
    Hits, occlusion and a frame must equal the oracle's bit for bit."""
    scene = T.scenes.cornell_scene()
    flat = scene.flatten(ctx)
    osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
    wb = osc.world_bound()
    rays = np.concatenate([camera_rays(T, ob, T.scenes.cornell_camera(96)), T.scenes.incoherent_rays(60000, wb[:3] - 0.3, wb[3:] + 0.3, seed=17)])
    rays[::97, 4] = 0.0  # some axis-parallel directions (every primitive is a candidate for those)
    t_ref, prim_ref, _, _ = osc.trace_closest(rays)
    occ_ref = osc.trace_any(rays)[0]
    cam = T.scenes.cornell_camera(32)
    ref, ref_L, _ = osc.render(cam, "path", 3, 6, seed=31, want_samples=True)
    ctx.set_option("leaf_sorted", 1)
    try:
        got = flat.trace_closest(rays)
        assert np.array_equal(got["prim"], prim_ref)
        assert_bits_equal(got["t"], t_ref, "t (leaf_sorted)")
        assert np.array_equal(flat.trace_any(rays), occ_ref)
        integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=31), 6)
        assert_bits_equal(integ.render(scene, ctx), ref, "film (leaf_sorted)")
        assert_bits_equal(integ.sample_radiance(scene), ref_L, "per-sample radiance (leaf_sorted)")
    finally:
        ctx.set_option("leaf_sorted", 0)
