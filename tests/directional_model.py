"""Scenes lit by a DirectionalLight and a composite model of their first vertex, built only from pinned pieces.

The oracle predates the light, so the model composes what it already answers: the camera (orc_generate_rays), the hit and its
geometry (orc_trace_closest), f (orc_bsdf_query), the point light (orc_light_query), visibility (orc_trace_any) and the sampler
(orc_sampler_u), with Float32 numpy in the reference's order of operations:
  Whitted      l += f * Li * abs(wi ⋅ n) / pdf for each light in order             integrators/sampler.jl:84-94
  Path, SPPM   one light picked by ceil(u * n); Ld = f * abs(wi ⋅ ns) * Li / pdf    integrators/sppm.jl:503-553
               divided by light_pdf = 1 / n
orc_bsdf_query re-normalises the tangent it is given, so where normalize(ss) != ss the model's frame is not the render's and a BSDF that
depends on the azimuth may differ in the last bits there: `direct_terms` returns which samples it reproduces exactly.
The directional light's part is directional.jl:39-47: Li = I, wi = direction, pdf = 1, shadow ray spawn_ray(p, p .+ direction .*
(2 * world_radius)) (Trace.jl:196-202), check_direction! (ray.jl:29) on its direction.
"""
import numpy as np

f32 = np.float32
BSDF_ALL, BSDF_SPECULAR = 31, 16
TS_DIM_VERTEX_BASE = 5


def box_triangles(lo, hi):
    """The 12 triangles of an axis-aligned box (vertices, 1-based indices), outward winding irrelevant here (two-sided shading)."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = [[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]]
    q = [(1, 2, 3, 4), (5, 8, 7, 6), (1, 5, 6, 2), (4, 3, 7, 8), (1, 4, 8, 5), (2, 6, 7, 3)]
    idx = []
    for a, b, c, d in q:
        idx += [a, b, c, a, c, d]
    return np.array(v, np.float32), np.array(idx, np.uint32)


def materials(T, kind):
    if kind == "matte":
        return (T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.8, 0.75, 0.7)), T.ConstantTexture(0.0)),
                T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.3, 0.5, 0.8)), T.ConstantTexture(20.0)))
    return (T.PlasticMaterial(T.ConstantTexture(T.RGBSpectrum(0.6, 0.5, 0.4)), T.ConstantTexture(T.RGBSpectrum(0.3)), T.ConstantTexture(0.1), True),
            T.PlasticMaterial(T.ConstantTexture(T.RGBSpectrum(0.2, 0.4, 0.7)), T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.05), True))


def sun(T, intensity=3.0):
    """A sun over the floor, from the front left; the translation of light_to_world must not matter (directional.jl:29)."""
    return T.DirectionalLight(T.translate([4.0, -7.0, 2.0]), T.RGBSpectrum(intensity, 0.9 * intensity, 0.8 * intensity), np.float32([-0.35, 1.0, 0.45]))


def floor_scene(T, material="matte", lights="sun", preprocessed=True, special=False):
    """A floor (axis-aligned: hit points lie on leaf-box faces) and a back wall, an occluding sphere and a triangle box (a shadow), lit by a
    directional light; `lights` = "sun", "point_first" (a point light before the sun) or "point_after".  special: a glass sphere and a mirror
    box beside them (full-depth tests)."""
    floor_m, obj_m = materials(T, material)
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    prims = []
    for p0, p1, p2, p3, n in (([0, 0, -2], [1, 0, -2], [1, 0, -3], [0, 0, -3], [0, 1, 0]), ([0, 0, -3], [1, 0, -3], [1, 1, -3], [0, 1, -3], [0, 0, 1])):
        for t in T.create_triangle_mesh(core, 2, np.array([1, 2, 3, 1, 3, 4], np.uint32), 4, [p0, p1, p2, p3], [n] * 4):
            prims.append(T.GeometricPrimitive(t, floor_m))
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.3, 0.22, -2.6]), False), 0.18, 360.0), obj_m))
    bv, bi = box_triangles([0.58, 0.0, -2.55], [0.82, 0.26, -2.3])
    for t in T.create_triangle_mesh(core, 12, bi, 8, bv):
        prims.append(T.GeometricPrimitive(t, obj_m))
    if special:
        glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0),
                                T.ConstantTexture(1.5), True)
        mirror = T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.9)))
        prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.5, 0.12, -2.2]), False), 0.1, 360.0), glass))
        mv, mi = box_triangles([0.1, 0.0, -2.95], [0.3, 0.5, -2.85])
        for t in T.create_triangle_mesh(core, 12, mi, 8, mv):
            prims.append(T.GeometricPrimitive(t, mirror))
    d = sun(T)
    point = T.PointLight(T.translate([0.2, 0.9, -2.1]), T.RGBSpectrum(1.5))
    ls = {"sun": [d], "point_first": [point, d], "point_after": [d, point]}[lights]
    scene = T.Scene(ls, T.BVHAccel(prims, 1))
    if preprocessed:
        T.preprocess(d, scene)
    return scene


def oracle_scene(T, ob, scene, bvh=None):
    """The scene inside the oracle, on the library's tree (or ``bvh``), with the lights the oracle knows (every light but the directional ones, in order)."""
    plain = T.Scene([l for l in scene.lights if not isinstance(l, T.DirectionalLight)], scene.aggregate)
    return ob.OracleScene.from_scene(plain, bvh=scene.flatten().bvh() if bvh is None else bvh)


def shadow_rays(light, p):
    """spawn_ray(p, outside_point) of the directional light's VisibilityTester, in the oracle's layout (o, t_max = Inf, d, time 0)."""
    two_r = f32(2.0) * f32(light.world_radius)
    d = np.asarray(light.direction, np.float32)
    p1 = (p + d[None, :] * two_r).astype(np.float32)
    dd = (p1 - p).astype(np.float32)
    o = (p + f32(1e-6) * dd).astype(np.float32)
    dd = np.where(dd == 0, f32(0.0), dd).astype(np.float32)  # check_direction!: -0 -> +0
    rays = np.zeros((p.shape[0], 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = o, np.inf, dd
    return rays


def first_vertex(T, ob, scene, cam, spp, seed, bvh=None):
    """Camera rays of every sample (sample-major, as trhip_last_sample_radiance lays them out) and the oracle's answers at their hits."""
    samples = T.scenes.camera_sample_grid(cam, spp, seed)
    rays = ob.generate_rays(cam, samples)
    osc = oracle_scene(T, ob, scene, bvh)
    _, prim, geom = osc.trace_closest(rays, want_geom=True)[:3]
    order = (scene.flatten().bvh() if bvh is None else bvh)[3]
    return samples, rays, osc, prim, geom, order


def material_ids(T, scene):
    """Oracle material id of every caller-order primitive (OracleScene.from_scene numbers the materials in first-use order)."""
    ids, out = {}, []
    for p in T.api.splice_nested(scene.aggregate.primitives):
        m = p.material
        if m is None:
            out.append(-1)
            continue
        if id(m) not in ids:
            ids[id(m)] = len(ids)
        out.append(ids[id(m)])
    return np.array(out, np.int64)


def _normalize_rows(w):
    n = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]).astype(np.float32)
    return ((np.float32(1.0) / n)[:, None] * w).astype(np.float32)  # normalize(v) = inv(norm(v)) * v  (oracle/orc_core.h:94-95)


def frame_is_reproducible(ss):
    """orc_bsdf_query builds the BSDF from the frame it is given and so normalises the tangent again (bsdf.jl: ss = normalize(∂p∂u)); the hit's ss is
    already normalize(∂p∂u).  Where normalising it twice moves a bit, the query's frame is not the render's, and a BSDF that depends on the
    azimuth (Oren-Nayar, microfacets) may differ in the last bit there: those hits are compared to 2 ulp instead of bit for bit."""
    return np.all(_normalize_rows(ss).view(np.uint32) == ss.view(np.uint32), axis=1)


def frame_free(T, scene):
    """Per oracle material id: a MatteMaterial with σ = 0 is one LambertianReflection lobe, whose f does not depend on the tangent frame."""
    ids, out = {}, []
    for p in T.api.splice_nested(scene.aggregate.primitives):
        m = p.material
        if m is not None and id(m) not in ids:
            ids[id(m)] = len(ids)
            out.append(isinstance(m, T.MatteMaterial) and float(T.api._tex_f(m.sigma)) == 0.0)
    return np.array(out + [False], bool)


def direct_terms(T, ob, scene, cam, spp, seed, integrator, bvh=None):
    """Per-sample radiance at max_depth = 1 (spp, h, w, 3) for "whitted" or "path" (also SPPM's camera-pass direct term, without β)."""
    samples, rays, osc, prim, geom, order = first_vertex(T, ob, scene, cam, spp, seed, bvh)
    mids = material_ids(T, scene)
    n = rays.shape[0]
    L = np.zeros((n, 3), np.float32)
    hit = np.nonzero(prim >= 0)[0]
    g = geom[hit]
    p, ng, ns, wo, ss = g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:12], g[:, 12:15]
    mat = mids[order[prim[hit]]]
    lights = scene.lights
    nl = len(lights)
    oracle_index = {}
    for k, l in enumerate(lights):
        if not isinstance(l, T.DirectionalLight):
            oracle_index[k] = len(oracle_index)
    # per light: Li, wi, pdf, visible at every hit
    per = []
    for k, l in enumerate(lights):
        if isinstance(l, T.DirectionalLight):
            Li = np.tile(np.asarray(l.i.c, np.float32), (hit.size, 1))
            wi = np.tile(np.asarray(l.direction, np.float32), (hit.size, 1))
            pdf = np.ones(hit.size, np.float32)
            vis = osc.trace_any(shadow_rays(l, p))[0] == 0
        else:
            q = np.empty((hit.size, 8), np.float32)
            ob.lib().orc_light_query(osc.h, oracle_index[k], ob.fp(np.ascontiguousarray(p)), hit.size, ob.fp(q))
            Li, wi, pdf, vis = q[:, 0:3], q[:, 3:6], q[:, 6], q[:, 7] != 0
        per.append((Li, wi, pdf, vis))

    def f_of(wi, flags, multi):
        out = np.zeros((hit.size, 3), np.float32)
        for m in np.unique(mat):
            sel = np.nonzero(mat == m)[0]
            frame = np.ascontiguousarray(np.concatenate([ng[sel], ns[sel], ss[sel]], axis=1))
            dirs = np.ascontiguousarray(np.concatenate([wo[sel], wi[sel]], axis=1))
            out[sel] = osc.bsdf_query(int(m), multi, 0, flags, frame, dirs)[:, :3]
        return out

    def absdot(a, b):
        return np.abs(((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(np.float32))[:, None]

    Lh = np.zeros((hit.size, 3), np.float32)
    if integrator == "whitted":
        for Li, wi, pdf, vis in per:
            f = f_of(wi, BSDF_ALL, False)
            ok = ~(np.all(Li == 0, axis=1) | (pdf == 0)) & ~np.all(f == 0, axis=1) & vis
            c = (((f * Li) * absdot(wi, ns)) / pdf[:, None]).astype(np.float32)
            Lh = np.where(ok[:, None], Lh + c, Lh).astype(np.float32)
    else:
        sb = cam.film.get_sample_bounds()
        w = int(sb.p_max[0] - sb.p_min[0]) + 1
        spp_i = hit // (n // spp)
        px = (int(sb.p_min[0]) + (hit % (n // spp)) % w).astype(np.int32)
        py = (int(sb.p_min[1]) + (hit % (n // spp)) // w).astype(np.int32)
        u = np.array([ob.lib().orc_sampler_u(seed, int(x), int(y), int(s), TS_DIM_VERTEX_BASE) for x, y, s in zip(px, py, spp_i)], np.float32)
        ln = np.clip(np.ceil(u * f32(nl)).astype(np.int64), 1, nl) if nl > 1 else np.ones(hit.size, np.int64)
        light_pdf = f32(1.0) / f32(nl)
        for k, (Li, wi, pdf, vis) in enumerate(per):
            f = (f_of(wi, BSDF_ALL & ~BSDF_SPECULAR, True) * absdot(wi, ns)).astype(np.float32)
            ok = (ln == k + 1) & (pdf > 0) & ~np.all(Li == 0, axis=1) & ~np.all(f == 0, axis=1) & vis
            Ld = (f32(0.0) + (f * Li) / pdf[:, None]).astype(np.float32)
            Ld = (Ld / light_pdf).astype(np.float32)
            Lh = np.where(ok[:, None], f32(0.0) + Ld, Lh).astype(np.float32)
    L[hit] = Lh
    exact = np.ones(n, bool)
    exact[hit] = frame_is_reproducible(np.ascontiguousarray(ss)) | frame_free(T, scene)[mat]
    sb = cam.film.get_sample_bounds()
    w, h = int(sb.p_max[0] - sb.p_min[0]) + 1, int(sb.p_max[1] - sb.p_min[1]) + 1
    return L.reshape(spp, h, w, 3), exact.reshape(spp, h, w)


def hit_points(T, ob, scene, cam, spp, seed):
    """World-space hit points of the camera rays (for the shadow rays of test 5)."""
    _, _, _, prim, geom, _ = first_vertex(T, ob, scene, cam, spp, seed)
    return np.ascontiguousarray(geom[prim >= 0, 0:3])
