"""Area lights in path frames on the GPU (trhip_emitters, trhip_render_path_emit; docs/design/29-path-emit.md), bit for bit against the model of tests/path_emit_model.py:
the sampler on its own over tables of 1, 2, 3, 32, 288 and 4232 emissive triangles (the last one searched in global memory); the emitted sums, the per-sample radiance,
the film and the frame's shadow-ray count over the parity matrix (seven scenes, two frame sizes, four depths, two scales, HITS_ONLY on and off); the identity (scale 0 is
trhip_render_path); the frames around an emit frame; the options the frame honours and the ones it ignores; the device variant, shards, a relit view served by the same
handle, and the refusals that need a context.

Shapes: tests/test_gpu_path_env.py's — a 5 x 3 crop under a filter of radius 1/2 at 1 spp (15 samples, fewer than one wave) and 37 x 29 under the default filter at 3 spp
(3627 samples: 56 full waves and a partial one; the all-materials scene's own 26 x 22 x 3).  What the frames contain is asserted from the model, never from the library's
output (tests/test_path_emit_api.py counts the branches over this matrix).  Every test runs the kernels on valid handles; the refusals end in an error code before any launch."""
import ctypes as C

import numpy as np
import pytest

import path_emit_model as em
import path_env_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
SEED = em.SEED
_sets = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def emitters(T, which):
    """The library's Emitters over the scene's emissive materials, one per process."""
    if which not in _sets:
        scene, _, radiance, _ = em.scene_of(T, which, committed=True)
        _sets[which] = T.Emitters(scene, {m: T.RGBSpectrum(*rgb) for m, rgb in radiance.items()})
    return _sets[which]


def check_frame(T, integ, scene, xyzw, ref, what):
    """Emitted sums, counted hits, samples, film and shadow-ray count of the frame just rendered against the model's result."""
    Lh, hits = integ.emitted(scene)
    assert_bits_equal(Lh, ref.Lh, "Lh: " + what)
    assert np.array_equal(hits, ref.hits), "counted hits: " + what
    assert_bits_equal(integ.sample_radiance(scene), pm.nan_rule(ref.Lp), "per-sample radiance: " + what)
    assert_bits_equal(xyzw, em.film(integ.camera, integ.sampler.samples_per_pixel, SEED, integ.sampler.sample_offset, ref.Lp), "film: " + what)
    assert integ.stats.shadow_rays == ref.delta_rays + ref.nee_rays, f"shadow rays {integ.stats.shadow_rays}, the model's {ref.delta_rays} + {ref.nee_rays}: " + what


# ---- the sampler on its own -------------------------------------------------------------------------------------------------------------------------------
def big_strip_scene(T):
    """heightfield_mesh(46) as a strip light: 4232 emissive triangles, a cdf of 4233 floats — more than the 16 KiB the kernel stages."""
    if "big" not in _sets:
        lamp = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0))
        prims, _ = T.scenes.cornell_primitives()
        _sets["big"] = (T.Scene([], T.BVHAccel(prims + em.strip_prims(T, 46, lamp), 1)), lamp)
    return _sets["big"]


@pytest.mark.parametrize("which", ["unlit_quad", "zero_area", "materials", "strip4", "strip12", "big"])
def test_the_sampler_equals_the_numpy_model(T, ob, ctx, which):
    if which == "big":
        scene, lamp = big_strip_scene(T)
        osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh())
        ids = em.material_ids(T, scene)
        tab = em.table(osc, {ids[id(lamp)]: em.LAMP}, len(ids))
        lib_set = T.Emitters(scene, {lamp: T.RGBSpectrum(*em.LAMP)})
    else:
        tab, lib_set = em.scene_of(T, which, committed=True)[3], emitters(T, which)
    n = tab.cdf.size - 1
    assert n == dict(unlit_quad=2, zero_area=3, materials=3, strip4=32, strip12=288, big=4232)[which] and lib_set.n_triangles == n
    u = em.edge_triples(4096, seed=n)
    j, y, pdf = em.sample(tab, u)
    gj, gy, gp = lib_set.sample(u)
    assert np.array_equal(gj, j), "the picked emitter"
    assert_bits_equal(gy, y, "the point")
    assert_bits_equal(gp, pdf, "P_j / A_j")
    assert (tab.area64[j] > 0).all()


def test_a_single_triangle_set(T, ob, ctx):
    """n = 1: the materials scene's lamp alone (its second emissive material is not listed)."""
    scene, osc, radiance, _ = em.scene_of(T, "materials", committed=True)
    lamp = next(m for m, rgb in radiance.items() if rgb == em.LAMP)
    ids = em.material_ids(T, scene)
    tab = em.table(osc, {ids[id(lamp)]: em.LAMP}, len(ids))
    one = T.Emitters(scene, {lamp: T.RGBSpectrum(*em.LAMP)})
    assert one.n_triangles == 1 and tab.cdf.tolist() == [0.0, 1.0]
    u = em.edge_triples(4096, seed=1)
    j, y, pdf = em.sample(tab, u)
    gj, gy, gp = one.sample(u)
    assert not gj.any() and np.array_equal(gj, j)
    assert_bits_equal(gy, y, "the point")
    assert_bits_equal(gp, pdf, "P_j / A_j")
    one.close()


# ---- the frame against the model --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", em.matrix(), ids=em.case_id)
def test_emitted_samples_film_and_ray_count_equal_the_model(T, ob, ctx, case):
    which, small, depth, scale, hits = case
    scene = em.scene_of(T, which, committed=True)[0]
    cam, spp = em.camera(T, small, which), 1 if small else 3
    ref = em.rendered(T, which, small, depth, scale, hits, committed=True)
    assert small or hits or ref.nee_rays > 500, "the frame casts emitter rays"
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    xyzw = integ.render(scene, emitters=emitters(T, which), emit_scale=scale, emit_hits_only=hits)
    check_frame(T, integ, scene, xyzw, ref, em.case_id(case))
    st = integ.stats
    assert st.camera_samples == ref.hits.size and st.max_depth_reached == depth and st.launches_shade == depth * st.n_batches


# ---- the identity -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cornell_quad", "strip4", "materials"])
def test_scale_zero_is_the_path_frame(T, ob, ctx, which):
    """With scale 0 every emitted term and every emitter ray's contribution is +0: film and samples are trhip_render_path's bit for bit, though the rays are cast."""
    scene = em.scene_of(T, which, committed=True)[0]
    cam = em.camera(T, False, which)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 8)
    film = integ.render(scene).copy()
    L = integ.sample_radiance(scene)
    path_rays = integ.stats.shadow_rays
    got = integ.render(scene, emitters=emitters(T, which), emit_scale=0.0)
    assert_bits_equal(got, film, "film")
    assert_bits_equal(integ.sample_radiance(scene), L, "samples")
    assert integ.stats.shadow_rays > path_rays + 1000, "the emitter rays are cast all the same"
    Lh, hits = integ.emitted(scene)
    assert not bits(Lh).any() and hits.sum() > 10
    got = integ.render(scene, emitters=emitters(T, which), emit_scale=0.0, emit_hits_only=True)
    assert_bits_equal(got, film, "film under HITS_ONLY")
    assert integ.stats.shadow_rays == path_rays, "HITS_ONLY casts no ray beyond the point lights'"
    assert_bits_equal(integ.render(scene), film, "the path frame after it")


# ---- neighbouring frames ----------------------------------------------------------------------------------------------------------------------------------
def test_frames_around_an_emit_frame_keep_their_bits(T, ob, ctx):
    """trhip_render_path, trhip_render_path_env_nee and trhip_render_ao on the same context, before and after an emit frame."""
    import path_nee_model as nm
    scene = em.scene_of(T, "strip4", committed=True)[0]
    cam = pm.camera(T)
    texels, _, R = nm.env_of(7, True)
    env = T.Environment(texels, R)
    path = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 4)
    ao = T.AmbientOcclusionIntegrator(cam, T.SeededSampler(3, seed=SEED), albedo=True, background=0.25)

    def all_three():
        out = []
        for integ, kw in ((path, {}), (path, dict(environment=env, env_scale=0.5, env_importance=0.25)), (ao, {})):
            out.append(integ.render(scene, **kw).copy())
            out.append(integ.sample_radiance(scene))
        return out

    before = all_three()
    assert path.render(scene, emitters=emitters(T, "strip4")).any()
    names = ("path film", "path samples", "path-env-nee film", "path-env-nee samples", "AO film", "AO samples")
    for got, ref, what in zip(all_three(), before, names):
        assert_bits_equal(got, ref, what + " after an emit frame")
    env.close()


# ---- options ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["radius-half", "default-filter"])
def test_option_sweep_against_one_reference(T, ob, ctx, small):
    """overlap, pipelines and batch_paths hold and change no bit; streaming and band_tile_rows are ignored; the fused and the sample-major record layout give the same
    records.  The 37 x 29 frame at batch_paths = 1209 (one sample pass of its 39 x 31 sample pixels) runs three batches, on one pipeline or two."""
    which, depth = "cornell_quad", 5
    scene = em.scene_of(T, which, committed=True)[0]
    cam, spp = em.camera(T, small, which), 1 if small else 3
    ref = em.rendered(T, which, small, depth, 0.5, False, committed=True)
    integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED), depth)
    defaults = dict(overlap=1, pipelines=1, batch_paths=0, streaming=0, film_fused=1, band_tile_rows=0)
    sweeps = [dict(), dict(overlap=0), dict(pipelines=2), dict(batch_paths=1209), dict(batch_paths=1209, pipelines=2), dict(batch_paths=1209, overlap=0), dict(streaming=1),
              dict(band_tile_rows=1), dict(film_fused=0), dict(film_fused=0, batch_paths=1209, pipelines=2, streaming=1)]
    try:
        for over in sweeps:
            for k, v in {**defaults, **over}.items():
                ctx.set_option(k, v)
            xyzw = integ.render(scene, emitters=emitters(T, which), emit_scale=0.5)
            check_frame(T, integ, scene, xyzw, ref, f"options {over}")
            if not small:
                assert integ.stats.n_batches == (3 if "batch_paths" in over or "pipelines" in over else 1), over
    finally:
        for k, v in defaults.items():
            ctx.set_option(k, v)


# ---- other behaviour --------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_device_variant_and_shards(T, ob, ctx):
    which = "strip12"
    scene = em.scene_of(T, which, committed=True)[0]
    cam = pm.camera(T)
    kw = dict(emitters=emitters(T, which), emit_scale=0.5)
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5)
    a = integ.render(scene, **kw).copy()
    La, (Lha, hits_a) = integ.sample_radiance(scene), integ.emitted(scene)
    assert hits_a.sum() > 100
    assert_bits_equal(integ.render(scene, **kw), a, "film, two calls")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples, two calls")
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 16).zero()
    assert integ.render(scene, device_out=d_film.ptr, **kw) is None
    assert_bits_equal(d_film.to_host(np.float32, (h, w, 4)), a, "device variant")
    assert_bits_equal(integ.sample_radiance(scene), La, "samples after the device variant")
    d_film.free()
    shards, lhs, films = [], [], []
    for spp, off in ((2, 0), (1, 2)):
        s = T.PathIntegrator(cam, T.SeededSampler(spp, seed=SEED, sample_offset=off), 5)
        films.append(s.render(scene, **kw).copy())
        shards.append(s.sample_radiance(scene))
        lhs.append(s.emitted(scene))
    assert_bits_equal(np.concatenate(shards), La, "(spp 2, offset 0) and (spp 1, offset 2) against (spp 3, offset 0)")
    assert_bits_equal(np.concatenate([l[0] for l in lhs]), Lha, "Lh of the shards")
    assert np.array_equal(np.concatenate([l[1] for l in lhs]), hits_a)
    # films are additive over sample_offset shards up to the order of addition: tests/test_gpu_path_env.py's bound, 48 addends per film pixel on either side
    total = films[0].astype(np.float64) + films[1].astype(np.float64)
    assert np.abs(total - a).max() <= 128 * 2.0 ** -23 * np.abs(a).max()


def test_a_relit_view_is_served_by_the_same_handle(T, ob, ctx):
    """The handle belongs to the committed geometry: Scene.with_lights' view of it renders with it, and equals the model of the scene built with those lights."""
    base = em.scene_of(T, "unlit_quad", committed=True)[0]
    lit = base.with_lights(T.scenes.cornell_lights())
    assert lit.flatten().geometry_id == base.flatten().geometry_id
    cam = em.camera(T, False, "cornell_quad")
    integ = T.PathIntegrator(cam, T.SeededSampler(3, seed=SEED), 5)
    xyzw = integ.render(lit, emitters=emitters(T, "unlit_quad"), emit_scale=0.5)
    # cornell_quad is unlit_quad's geometry under the Cornell box's light; the oracle walks the tree THIS geometry was committed with
    osc = ob.OracleScene.from_scene(em.scene_of(T, "cornell_quad")[0], bvh=base.flatten().bvh())
    tab = em.scene_of(T, "unlit_quad", committed=True)[3]
    ref = em.shade(em.walk(osc, cam, 3, 5, SEED, 0, tab, 0.5, False))
    assert ref.delta_rays > 1000 and ref.nee_rays > 1000
    check_frame(T, integ, lit, xyzw, ref, "the relit view")


def test_refusals_with_a_context(T, ob, ctx):
    import test_gpu_sky as tgs
    scene = em.scene_of(T, "cornell_quad", committed=True)[0]
    flat, cam, L = scene.flatten(), pm.camera(T, True), T.lib()
    sn, st, out = cam.sensor(), T.Stats(), np.zeros((3, 5, 4), F)
    h_em = emitters(T, "cornell_quad")._h

    def params(**over):
        p = T._ffi.PathEmitParams()
        assert L.trhip_path_emit_default_params(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, spp=1, depth=3, scene_h=flat._h, sensor=sn, outp=T._ffi.fptr(out), context=ctx._h, em_h=h_em):
        return L.trhip_render_path_emit(context, scene_h, C.byref(sensor) if sensor is not None else None, spp, depth, SEED, 0, em_h, C.byref(p) if p is not None else None, outp, C.byref(st))

    assert call(params()) == 0 and out.any()
    for over, word in ((dict(scale=-0.5), b"scale"), (dict(flags=2), b"flag")):
        assert call(params(**over)) == -1 and word in L.trhip_last_error(ctx._h), over
    # the parameter block before trhip_render_path's refusals, those before the emitters'
    assert call(params(flags=4), spp=0, em_h=None) == -1 and b"flag" in L.trhip_last_error(ctx._h)
    assert call(params(), spp=0, em_h=None) == -1 and b"spp" in L.trhip_last_error(ctx._h)
    assert call(params(), depth=0, em_h=None) == -1 and b"max_depth" in L.trhip_last_error(ctx._h)
    assert call(None) == -1 and call(params(), outp=None) == -1 and call(params(), scene_h=None) == -1 and call(params(), sensor=None) == -1 and call(params(), context=None) == -1
    assert call(params(), em_h=None) == -1 and b"null emitters" in L.trhip_last_error(ctx._h)
    assert L.trhip_render_path_emit_device(ctx._h, flat._h, C.byref(sn), 1, 3, SEED, 0, h_em, C.byref(params()), None, C.byref(st)) == -1
    holes = tgs.materialless(T)  # material-less primitives: trhip_render_path's refusal, before the emitters are looked at
    assert call(params(), scene_h=holes.flatten()._h, em_h=None) == -3 and b"material-less" in L.trhip_last_error(ctx._h)
    # emitters of another geometry: the same description committed again is another geometry
    other_scene = em.build_scene(T, "cornell_quad")[0]
    assert call(params(), scene_h=other_scene.flatten()._h) == -1 and b"another committed geometry" in L.trhip_last_error(ctx._h)
    rec = np.zeros(15 * 4, F)
    assert call(params()) == 0 and L.trhip_last_emitted(ctx._h, T._ffi.fptr(rec), rec.size) == 0
    assert L.trhip_last_emitted(ctx._h, T._ffi.fptr(rec), rec.size - 4) == -1
    T.PathIntegrator(cam, T.SeededSampler(1, seed=SEED), 3).render(scene)
    assert L.trhip_last_emitted(ctx._h, T._ffi.fptr(rec), rec.size) == -1 and b"not an emit frame" in L.trhip_last_error(ctx._h)
    other = T.Context(0)  # a second context on the same GPU: its emitters are not this context's
    try:
        s2, rad2 = em.build_scene(T, "unlit_quad")
        theirs = T.Emitters(s2, {m: T.RGBSpectrum(*rgb) for m, rgb in rad2.items()}, ctx=other)
        assert call(params(), em_h=theirs._h) == -1 and b"another context" in L.trhip_last_error(ctx._h)
        assert call(params()) == 0
        theirs.close()
        s2.flatten(other).free()  # the scene on the second context goes before its context does
    finally:
        other.close()


def test_emitters_create_refusals_in_order(T, ob, ctx):
    scene, _, radiance, _ = em.scene_of(T, "cornell_quad", committed=True)
    flat, L = scene.flatten(), T.lib()
    ids_of = em.material_ids(T, scene)
    lamp = next(iter(radiance))
    lamp_id = ids_of[id(lamp)]
    h = C.c_void_p()

    def create(ids, le, n=None, scene_h=flat._h, context=ctx._h):
        ids, le = np.asarray(ids, np.uint32), np.ascontiguousarray(le, F)
        return L.trhip_emitters_create(context, scene_h, T._ffi.u32ptr(ids), T._ffi.fptr(le), ids.size if n is None else n, C.byref(h))

    assert create([lamp_id], [1, 1, 1], n=0) == -1 and b"n_materials" in L.trhip_last_error(ctx._h)
    for bad in ([-1, 1, 1], [1, np.inf, 1], [1, 1, np.nan]):
        assert create([999], bad) == -1 and b"radiance" in L.trhip_last_error(ctx._h), "the radiance before the material ids"
    fresh = C.c_void_p()
    assert L.trhip_scene_new(ctx._h, C.byref(fresh)) == 0
    assert create([999], [1, 1, 1], scene_h=fresh) == -1 and b"not committed" in L.trhip_last_error(ctx._h), "the scene before the material ids"
    L.trhip_scene_free(fresh)
    assert create([999], [1, 1, 1]) == -1 and b"not defined" in L.trhip_last_error(ctx._h)
    assert create([lamp_id, lamp_id], [[1, 1, 1], [2, 2, 2]]) == -1 and b"twice" in L.trhip_last_error(ctx._h)
    prims = T.api.splice_nested(scene.aggregate.primitives)
    on_sphere = next(ids_of[id(p.material)] for p in prims if isinstance(p.shape, T.Sphere))
    assert create([lamp_id, on_sphere], [[0, 0, 0], [1, 1, 1]]) == -3 and b"sphere" in L.trhip_last_error(ctx._h), "the sphere before the weights"
    assert create([lamp_id], [0, 0, 0]) == -1 and b"nothing to sample" in L.trhip_last_error(ctx._h)
    assert not h.value
    with pytest.raises(T.TraceHipError, match="no primitive with this"):
        T.Emitters(scene, {T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0)): T.RGBSpectrum(1.0)})
    with pytest.raises(T.TraceHipError, match="cannot be combined"):
        T.PathIntegrator(pm.camera(T, True), T.SeededSampler(1, seed=SEED), 3).render(scene, emitters=emitters(T, "cornell_quad"), environment=T.Environment.constant((1, 1, 1)))
