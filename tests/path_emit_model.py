"""The model of an emit frame (trhip_emitters, trhip_render_path_emit; docs/design/29-path-emit.md), from the oracle and numpy alone.  tests/host/path_emit_oracle.cpp — the
oracle's API unit, included unchanged, plus path_li restated with the emitted term and every vertex's next-event estimate towards the emitters — is compiled here as
tests/path_nee_model.py compiles its helper.  The table is built HERE, in numpy Float64 with every sum in the specification's order, from the world-space vertices the oracle's
committed tree holds; pick and point are restated in numpy Float32 (the C++ ones are pinned to them by tests/test_path_emit_api.py); numpy finishes the frame in depth order,
one Float32 operation per step:

    L = (L + delta_v) + c_v  for v = 0, 1, …     Lh = Lh + t_v  for v = 0, 1, …     L' = L + Lh

Nothing here calls the library under test."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
from collections import namedtuple

import numpy as np

import oracle_bridge as ob
import path_env_model as pm

F = np.float32
ROOT = pm.ROOT
_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
_I32 = C.POINTER(C.c_int32)
_lib = None
V_NONE, V_SPECULAR, V_NEE, V_HITS_ONLY = 0, 1, 2, 3
R_NO_RAY, R_BLACK, R_OPEN, R_OCCLUDED = 0, 1, 2, 3
E_NONE, E_COUNTED, E_SUPPRESSED = 0, 1, 2
HITS_ONLY = 1
TS_DIM_EMIT_BASE = 517  # include/trace_sampler.h
ONE_MINUS = F(1.0) - F(2.0 ** -24)

Table = namedtuple("Table", "tri cdf mat_le slots area64")
Result = namedtuple("Result", "L Lh hits Lp c cast open nee_rays delta_rays classes")


def lib():
    global _lib
    if _lib is None:
        ob.lib()  # liboracle.so first: its scenes are what this library walks
        cxx, flags = pm.makefile_flags()
        d = tempfile.mkdtemp(prefix="path_emit_oracle_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libpath_emit_oracle.so")
        subprocess.check_call([cxx] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "host", "path_emit_oracle.cpp")])
        l = C.CDLL(so)
        l.path_emit_vertex_floats.restype = C.c_int
        l.path_emit_prims.restype = C.c_int
        l.path_emit_prims.argtypes = [C.c_void_p, _F, _I32, _I32]
        l.path_emit_sample.restype = None
        l.path_emit_sample.argtypes = [_F, _F, C.c_uint32, _F, C.c_int64, _U32, _F, _F]
        l.path_emit_walk.restype = C.c_int
        l.path_emit_walk.argtypes = [C.c_void_p, C.POINTER(ob.OrcSensor), C.c_int64, C.c_int, C.c_uint64, C.c_uint32, _F, _F, C.c_uint32, _F, C.c_int, C.c_float, C.c_uint32, _F]
        assert l.path_emit_vertex_floats() == 16
        _lib = l
    return _lib


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------------
def prims_of(osc):
    """Per ordered slot of the oracle's committed tree: world vertices (n, 9) Float32, material (n,) int32 (-1: none), kind (n,) int32 (0 triangle, 1 sphere)."""
    n = int(ob.lib().orc_scene_prim_count(osc.h))
    v, m, k = np.zeros((n, 9), F), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert lib().path_emit_prims(osc.h, ob.fp(v), m.ctypes.data_as(_I32), k.ctypes.data_as(_I32)) == 0
    return v, m, k


def table_from_triangles(v9, le3, slots=None, n_materials=0, materials=None):
    """The table over the given emissive triangles, in the given order: v9 (n, 9) Float32 world vertices, le3 (n, 3) Float32 the radiance of each one's material.
    A64 = 1/2 |(p1 - p0) x (p2 - p0)| in Float64 from the Float32 vertices, weight = A64 * ((Le.r + Le.g) + Le.b), total = the weights added in order j = 0, 1, …;
    cdf[j] = Float32(acc_j / total) with acc_j the sum of the weights before j, cdf[n] = 1; P_j = cdf[j + 1] - cdf[j] in Float32, A_j = Float32(A64_j)."""
    v = np.asarray(v9, F).astype(np.float64).reshape(-1, 3, 3)
    le = np.asarray(le3, F).reshape(-1, 3)
    n = v.shape[0]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    a64 = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    w = a64 * ((le[:, 0].astype(np.float64) + le[:, 1].astype(np.float64)) + le[:, 2].astype(np.float64))
    acc = np.cumsum(w)  # (sequential: acc[j] = acc[j - 1] + w[j])
    total = acc[-1]
    assert total > 0, "no triangle with positive weight"
    cdf = np.empty(n + 1, F)
    cdf[0] = F(0.0)
    cdf[1:n] = (acc[:n - 1] / total).astype(F)
    cdf[n] = F(1.0)
    tri = np.zeros((n, 16), F)
    vf = np.asarray(v9, F).reshape(-1, 9)
    tri[:, 0:3], tri[:, 4:7], tri[:, 8:11] = vf[:, 0:3], vf[:, 3:6], vf[:, 6:9]
    tri[:, 3] = cdf[1:] - cdf[:-1]
    tri[:, 7] = a64.astype(F)
    sl = np.arange(n, dtype=np.uint32) if slots is None else np.asarray(slots, np.uint32)
    tri[:, 11] = sl.view(F)
    tri[:, 12:15] = le
    mat_le = np.zeros((max(n_materials, 1), 4), F)
    for mid, rgb in (materials or {}).items():
        mat_le[mid, 0:3] = F(rgb)
    return Table(tri=np.ascontiguousarray(tri), cdf=cdf, mat_le=mat_le, slots=sl, area64=a64)


def table(osc, radiance_by_material_id, n_materials):
    """The emitter set of a committed oracle scene: every triangle whose material id is a key of `radiance_by_material_id` (id -> rgb), in ascending slot."""
    v, m, k = prims_of(osc)
    for mid in radiance_by_material_id:
        assert not ((k == 1) & (m == mid)).any(), "a listed material on a sphere"
    on = (k == 0) & np.isin(m, list(radiance_by_material_id))
    slots = np.nonzero(on)[0].astype(np.uint32)
    le = np.array([radiance_by_material_id[int(x)] for x in m[on]], F).reshape(-1, 3)
    return table_from_triangles(v[on], le, slots, n_materials, radiance_by_material_id)


def pick(cdf, xi):
    """The largest j in [0, n - 1] with cdf[j] <= xi, by the device's fixed number of steps."""
    cdf, xi = np.asarray(cdf, F), np.asarray(xi, F)
    n = cdf.size - 1
    lo = np.zeros(xi.shape, np.int64)
    step = 1 << ((n - 1).bit_length() - 1) if n > 1 else 0
    while step:
        k = lo + step
        ok = k <= n - 1
        take = ok & (cdf[np.where(ok, k, 0)] <= xi)
        lo = np.where(take, k, lo)
        step >>= 1
    return lo.astype(np.uint32)


def point(p0, p1, p2, u0, u1):
    """s = sqrt(u0), b0 = 1 - s, b1 = u1 s, b2 = (1 - b0) - b1, y = (b0 p0 + b1 p1) + b2 p2: one Float32 operation per step."""
    u0, u1 = np.asarray(u0, F), np.asarray(u1, F)
    s = np.sqrt(u0)
    b0 = F(1.0) - s
    b1 = u1 * s
    b2 = (F(1.0) - b0) - b1
    y = (b0[..., None] * p0 + b1[..., None] * p1) + b2[..., None] * p2
    assert y.dtype == F
    return y


def sample(tab, u3):
    """(index, point, P_j / A_j) for every triple (xi, u0, u1): what trhip_emitters_sample returns."""
    u = np.asarray(u3, F).reshape(-1, 3)
    j = pick(tab.cdf, u[:, 0])
    r = tab.tri[j]
    with np.errstate(all="ignore"):
        return j, point(r[:, 0:3], r[:, 4:7], r[:, 8:11], u[:, 1], u[:, 2]), r[:, 3] / r[:, 7]


def sample_cpp(tab, u3):
    """The same through tests/host/path_emit_oracle.cpp's pick and point."""
    u = np.ascontiguousarray(np.asarray(u3, F).reshape(-1, 3))
    n = u.shape[0]
    j, y, p = np.empty(n, np.uint32), np.empty((n, 3), F), np.empty(n, F)
    lib().path_emit_sample(ob.fp(tab.tri), ob.fp(tab.cdf), tab.cdf.size - 1, ob.fp(u), n, j.ctypes.data_as(_U32), ob.fp(y), ob.fp(p))
    return j, y, p


def edge_triples(count=4096, seed=11):
    """`count` triples of [0, 1)^3: every combination of xi, u0, u1 in {0, 1 - 2^-24} first, then random 24-bit numbers."""
    rng = np.random.default_rng(seed)
    u = (rng.integers(0, 1 << 24, size=(count, 3)).astype(np.float64) * 2.0 ** -24).astype(F)
    e = (F(0.0), ONE_MINUS)
    u[:8] = [(a, b, c) for a in e for b in e for c in e]
    return u


def random_table(n, seed=5):
    """A table over n random triangles — no scene —, every fifth one of zero area and one material black."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, size=(n, 9)).astype(F)
    v[::5, 6:9] = v[::5, 3:6]  # p2 = p1
    le = np.tile(F([3.0, 2.0, 1.0]), (n, 1))
    le[1::7] = F(0.0)
    if n == 1:
        v[0] = F([0, 0, 0, 1, 0, 0, 0, 1, 0])
        le[0] = F([1, 1, 1])
    elif n <= 3:
        v[n - 1] = F([0, 0, 0, 1, 0, 0, 0, 1, 0])
        le[n - 1] = F([1, 2, 3])
    return table_from_triangles(v, le)


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------------------------
def walk(osc, cam, spp, max_depth, seed, sample_offset, tab, scale, hits_only):
    shape = pm.sample_shape(cam, spp)
    vtx = np.empty(shape + (max_depth, 16), F)
    sn = ob.make_sensor(cam)
    rc = lib().path_emit_walk(osc.h, C.byref(sn), spp, max_depth, seed, sample_offset, ob.fp(tab.tri), ob.fp(tab.cdf), tab.cdf.size - 1, ob.fp(tab.mat_le), tab.mat_le.shape[0], F(scale),
                              HITS_ONLY if hits_only else 0, ob.fp(vtx))
    assert rc == 0, "scene not committed"
    return vtx


def shade(vtx):
    """The frame from its walk.  L: the path's own radiance (point lights and emitter rays in depth order, raw), Lh: the emitted sum, hits: the counted hits, Lp = L + Lh
    (raw: the NaN rule is the film pass's and trhip_last_sample_radiance's)."""
    D = vtx.shape[-2]
    state, verdict, em = vtx[..., 0].astype(np.int32), vtx[..., 1].astype(np.int32), vtx[..., 15].astype(np.int32)
    c, beta = vtx[..., 2:5], vtx[..., 5:8]
    nee = state == V_NEE
    cast = nee & (verdict >= R_OPEN)
    is_open = cast & (verdict == R_OPEN)
    L = np.zeros(vtx.shape[:-2] + (3,), F)
    Lh = np.zeros_like(L)
    with np.errstate(all="ignore"):
        for v in range(D):
            L = L + vtx[..., v, 8:11]  # the point-light addend beta * uniform_sample_one_light: +0 where it estimates nothing
            o = is_open[..., v]
            L[o] = L[o] + c[..., v, :][o]
            # an occluded ray adds beta * 0: NaN in the channels where beta is not finite (the shadow queue's poison bits), nothing otherwise
            bad = (cast[..., v] & ~o)[..., None] & ~np.isfinite(beta[..., v, :])
            L[bad] = F(np.nan)
            k = em[..., v] == E_COUNTED
            Lh[k] = Lh[k] + vtx[..., v, 12:15][k]
        Lp = L + Lh
    assert L.dtype == Lh.dtype == Lp.dtype == F
    counted = em == E_COUNTED
    prev_spec = np.zeros(state.shape, bool)
    prev_spec[..., 1:] = state[..., :-1] == V_SPECULAR
    first = np.zeros(state.shape, bool)
    first[..., 0] = True
    last = np.zeros(state.shape, bool)
    last[..., D - 1] = True
    classes = dict(
        counted_depth1=int((counted & first).sum()), counted_after_specular=int((counted & prev_spec & ~first).sum()), suppressed=int((em == E_SUPPRESSED).sum()),
        open=int(is_open.sum()), occluded=int((cast & ~is_open).sum()), no_ray_fa=int((nee & (verdict == R_BLACK)).sum()), no_ray_geometry=int((nee & (verdict == R_NO_RAY)).sum()),
        at_max_depth=int((cast & last).sum()), specular=int((state == V_SPECULAR).sum()), hits_only_vertices=int((state == V_HITS_ONLY).sum()))
    return Result(L=L, Lh=Lh, hits=counted.sum(axis=-1).astype(np.int32), Lp=Lp, c=c, cast=cast, open=is_open, nee_rays=int(cast.sum()), delta_rays=int(vtx[..., 11].sum()), classes=classes)


film = pm.film  # the oracle's film tiles over the samples L' after the NaN rule

# ---- the cases the two test files share (tests/test_path_emit_api.py, tests/test_gpu_path_emit.py) ---------------------------------------------------------------------
SEED = pm.SEED
DEPTHS = pm.DEPTHS
SCENE_NAMES = ("cornell_quad", "unlit_quad", "strip1", "strip4", "strip12", "materials", "zero_area")
COMBOS = ((0.5, False), (0.5, True), (0.0, False), (0.0, True))  # (scale, HITS_ONLY)
LAMP = (17.0, 12.0, 4.0)
SECOND = (0.5, 2.0, 6.0)
_cache = {}


def _matte(T, k):
    return T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(k)), T.ConstantTexture(0.0))


def quad_prims(T, material, x0=0.35, x1=0.65, y=0.999, z0=-2.35, z1=-2.65, extra_zero_area=False):
    """A horizontal quad facing down (two triangles), optionally with a third triangle of zero area (three collinear corners) in the same mesh."""
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    v = [[x0, y, z0], [x0, y, z1], [x1, y, z1], [x1, y, z0]]
    idx = [1, 2, 3, 1, 3, 4]
    if extra_zero_area:
        v.append([(x0 + x1) / 2, y, z0])
        idx += [1, 4, 5]
    mesh = T.create_triangle_mesh(core, len(idx) // 3, np.uint32(idx), len(v), F(v), F([[0, -1, 0]] * len(v)))
    return [T.GeometricPrimitive(t, material) for t in mesh]


def strip_prims(T, n, material):
    """heightfield_mesh(n) narrowed to a strip and lifted under the ceiling, with its own material: 2 n^2 emissive triangles."""
    verts, idx, nrm = T.scenes.heightfield_mesh(n)
    v = np.array(verts, F)
    v[:, 0] = F(0.35) + F(0.3) * v[:, 0]
    v[:, 1] = v[:, 1] + F(0.8)
    return [T.create_mesh_primitives(T.ShapeCore(T.translate([0, 0, 0]), False), idx, v, nrm, material)]


def build_scene(T, which):
    """(scene, {material object: rgb})"""
    lamp = _matte(T, 0.5)
    if which == "cornell_quad":
        prims, _ = T.scenes.cornell_primitives()
        return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims + quad_prims(T, lamp), 1)), {lamp: LAMP}
    if which == "unlit_quad":
        prims, _ = T.scenes.cornell_primitives()
        return T.Scene([], T.BVHAccel(prims + quad_prims(T, lamp), 1)), {lamp: LAMP}
    if which == "zero_area":
        prims, _ = T.scenes.cornell_primitives()
        return T.Scene([], T.BVHAccel(prims + quad_prims(T, lamp, extra_zero_area=True), 1)), {lamp: LAMP}
    if which.startswith("strip"):
        base = T.scenes.mesh_scene(16)
        return T.Scene(base.lights, T.BVHAccel(list(base.aggregate.primitives) + strip_prims(T, int(which[5:]), lamp), 1)), {lamp: LAMP}
    if which == "materials":  # the all-materials scene with a one-triangle emitter and a second emissive material of another colour
        import shade_variants as sv
        base = sv.build(T, tangents=False, sun="none")[0]
        second = _matte(T, 0.25)
        core = T.ShapeCore(T.translate([0, 0, 0]), False)
        one = T.create_triangle_mesh(core, 1, np.uint32([1, 2, 3]), 3, F([[0.3, 0.97, -2.3], [0.5, 0.97, -2.7], [0.7, 0.97, -2.3]]), F([[0, -1, 0]] * 3))
        prims = list(base.aggregate.primitives) + [T.GeometricPrimitive(t, lamp) for t in one] + quad_prims(T, second, 0.02, 0.12, 0.5, -2.2, -2.6)
        return T.Scene(base.lights, T.BVHAccel(prims, 1)), {lamp: LAMP, second: SECOND}
    if which == "grey_box":  # all matte, no point light: tests/path_nee_model.py's grey box on open ground, under a small bright quad above the camera's window (no camera ray
        # meets it: what the frame shows of it is what it lights)
        import path_nee_model as nm
        base = nm.grey_box_scene(T)
        return T.Scene([], T.BVHAccel(list(base.aggregate.primitives) + quad_prims(T, lamp, 0.2, 0.4, 1.5, -2.3, -2.5), 1)), {lamp: (400.0, 400.0, 400.0)}
    raise KeyError(which)


def material_ids(T, scene):
    """{id(material object): material id}: ids in order of first appearance over the spliced primitives, as FlatScene and OracleScene.from_scene both assign them."""
    ids = {}
    for p in T.api.splice_nested(scene.aggregate.primitives):
        if p.material is not None and id(p.material) not in ids:
            ids[id(p.material)] = len(ids)
    return ids


def scene_of(T, which, committed=False):
    """(scene, oracle scene, {material object: rgb}, table), built once per process and left alone.  committed: the oracle walks the tree the library committed (the
    GPU tests: needs a device); otherwise the oracle's own construction of the reference's tree."""
    if ("scene", which, committed) not in _cache:
        scene, radiance = build_scene(T, which)
        osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh() if committed else None)
        ids = material_ids(T, scene)
        tab = table(osc, {ids[id(m)]: rgb for m, rgb in radiance.items()}, len(ids))
        for a in (tab.tri, tab.cdf, tab.mat_le):
            a.setflags(write=False)
        _cache["scene", which, committed] = (scene, osc, radiance, tab)
    return _cache["scene", which, committed]


def camera(T, small, which):
    return pm.camera(T, small, "materials" if which == "materials" else None)


def matrix():
    """The parity matrix: (scene, small, depth, scale, hits_only).  Every scene x size x depth once, and within every scene x size both scales with HITS_ONLY off and on: a
    covering arrangement of 56 frames, not the full product of 224 (test_path_emit_api.py checks the cover)."""
    cases = []
    g = 0
    for which in SCENE_NAMES:
        for small in (True, False):
            for di, depth in enumerate(DEPTHS):
                scale, hits = COMBOS[(di + g) % 4]
                cases.append((which, small, depth, scale, hits))
            g += 1
    return cases


def case_id(c):
    which, small, depth, scale, hits = c
    return "%s-%s-d%d-s%g-%s" % (which, "5x3" if small else "full", depth, scale, "hits" if hits else "nee")


def rendered(T, which, small, max_depth, scale, hits_only, committed=False, spp=None, sample_offset=0):
    """shade(walk()) of a case, computed once per process and shared (read-only)."""
    key = ("frame", which, small, max_depth, scale, hits_only, committed, spp, sample_offset)
    if key not in _cache:
        _, osc, _, tab = scene_of(T, which, committed)
        n = spp if spp is not None else (1 if small else 3)
        r = shade(walk(osc, camera(T, small, which), n, max_depth, SEED, sample_offset, tab, scale, hits_only))
        for a in (r.L, r.Lh, r.Lp):
            a.setflags(write=False)
        _cache[key] = r
    return _cache[key]
