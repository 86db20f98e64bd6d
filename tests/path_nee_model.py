"""The model of a path-env frame with next-event estimation (trhip_render_path_env_nee; docs/design/28-path-nee.md), from the oracle and the numpy models alone.
tests/host/path_nee_oracle.cpp — the oracle's API unit, included unchanged, plus path_li restated with the escape record, its mark and the geometry of every vertex's estimate —
is compiled here as tests/path_env_model.py compiles its helper.  A map-chosen direction depends on (u0, u1) alone: tests/sky_is_model.py's env_sample computes it for every
(sample, vertex) up front, the C++ walk takes those directions, and numpy finishes with env_pdf, env_eval and the sums in depth order, one Float32 operation per step:

    p = om pb + mix pe,   ce = E(wi) * scale,   t = fa * ce,   Ld = t / p,   c = beta * Ld,   L = (L + delta_v) + c_v  for v = 0, 1, …,   L' = L + beta_esc * (E(dir) * scale)

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

import ao_model as am
import oracle_bridge as ob
import path_env_model as pm
import sky_is_model as im
import sky_model as sm

F = np.float32
ROOT = pm.ROOT
_F = C.POINTER(C.c_float)
_lib = None
V_NONE, V_SPECULAR, V_MAP, V_BSDF = 0, 1, 2, 3
R_NO_DIRECTION, R_BLACK, R_OPEN, R_OCCLUDED = 0, 1, 2, 3
TS_V_LIGHT_U0, TS_V_LIGHT_U1 = 1, 2  # include/trace_sampler.h

Walk = namedtuple("Walk", "L rec vtx mix max_depth")
Result = namedtuple("Result", "L Lp rec c cast open nee_rays delta_rays classes")


def ts_vertex_dim(v, slot):
    return 5 + 8 * v + slot


def lib():
    global _lib
    if _lib is None:
        ob.lib()  # liboracle.so first: its scenes are what this library walks
        cxx, flags = pm.makefile_flags()
        d = tempfile.mkdtemp(prefix="path_nee_oracle_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libpath_nee_oracle.so")
        subprocess.check_call([cxx] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "host", "path_nee_oracle.cpp")])
        l = C.CDLL(so)
        l.path_nee_vertex_floats.restype = C.c_int
        l.path_nee_walk.restype = C.c_int
        l.path_nee_walk.argtypes = [C.c_void_p, C.POINTER(ob.OrcSensor), C.c_int64, C.c_int, C.c_uint64, C.c_uint32, C.c_float, _F, _F, _F, _F]
        assert l.path_nee_vertex_floats() == 16
        _lib = l
    return _lib


def env_directions(cam, spp, max_depth, seed, sample_offset, tab, R=None):
    """env_sample of every (sample, vertex)'s (TS_V_LIGHT_U0, TS_V_LIGHT_U1): (n, max_depth, 3) Float32, samples in the walk's order."""
    S = sys.modules["trace_jl_amd"].scenes
    key, _, _ = am.sample_keys(cam, spp, seed, sample_offset)
    out = np.empty((key.size, max_depth, 3), F)
    for v in range(max_depth):
        out[:, v] = im.env_sample(tab, S.ts_uniform(key, ts_vertex_dim(v, TS_V_LIGHT_U0)), S.ts_uniform(key, ts_vertex_dim(v, TS_V_LIGHT_U1)), R)
    return out


def walk(osc, cam, spp, max_depth, seed, sample_offset, mix, tab, R=None):
    """The walk: everything of the frame that does not depend on scale, the flag and the map's texels (the tables and the matrix it does depend on)."""
    shape = pm.sample_shape(cam, spp)
    dirs = np.ascontiguousarray(env_directions(cam, spp, max_depth, seed, sample_offset, tab, R))
    L, rec, vtx = np.empty(shape + (3,), F), np.empty(shape + (8,), F), np.empty(shape + (max_depth, 16), F)
    sn = ob.make_sensor(cam)
    rc = lib().path_nee_walk(osc.h, C.byref(sn), spp, max_depth, seed, sample_offset, F(mix), ob.fp(dirs), ob.fp(L), ob.fp(rec), ob.fp(vtx))
    assert rc == 0, "scene not committed"
    return Walk(L=L, rec=rec, vtx=vtx, mix=F(mix), max_depth=max_depth)


def shade(w, texels, tab, R=None, scale=1.0, hide_background=False):
    """The frame from its walk.  L: the raw radiance before the escape (point lights and NEE in depth order), Lp: with the counted escape (raw: the NaN rule is the film
    pass's and trhip_last_sample_radiance's), c: every vertex's NEE contribution (zero where no ray is cast), cast / open: where a ray is cast / reaches nothing,
    nee_rays / delta_rays: the frame's shadow rays of either kind, classes: the counts tests/test_path_nee_api.py asserts on."""
    mix, om = F(w.mix), F(1.0) - F(w.mix)
    vtx = w.vtx
    D = w.max_depth
    state, verdict = vtx[..., 0].astype(np.int32), vtx[..., 1].astype(np.int32)
    has_dir = (state >= V_MAP) & (verdict != R_NO_DIRECTION)
    wi, pb, fa, beta = vtx[..., 2:5], vtx[..., 5], vtx[..., 6:9], vtx[..., 9:12]
    flat = wi.reshape(-1, 3)
    with np.errstate(all="ignore"):
        pe = im.env_pdf(tab, flat, R).reshape(pb.shape)
        p = om * pb + mix * pe
        positive = has_dir & (p > 0)
        cast = positive & (verdict >= R_OPEN)
        ce = (sm.env_eval(texels, flat, R) * F(scale)).reshape(wi.shape)
        t = fa * ce
        Ld = t / np.where(cast, p, F(1.0))[..., None]
        c = (beta * Ld).astype(F)
        c[~cast] = F(0.0)
        is_open = cast & (verdict == R_OPEN)
        L = np.zeros(vtx.shape[:-2] + (3,), F)
        for v in range(D):
            L = L + vtx[..., v, 12:15]  # the point-light addend beta * uniform_sample_one_light: +0 where it estimates nothing
            o = is_open[..., v]
            L[o] = L[o] + c[..., v, :][o]
            # an occluded ray adds beta * 0: NaN in the channels where beta is not finite (the shadow queue's poison bits), nothing otherwise
            bad = (cast[..., v] & ~o)[..., None] & ~np.isfinite(beta[..., v, :])
            L[bad] = F(np.nan)
    assert L.dtype == F and c.dtype == F
    rec = w.rec
    depth, mark = rec[..., 3], rec[..., 7]
    counted = (depth != 0) & (mark == 0) & ~((depth == 1) & bool(hide_background))
    Lp = L.copy()
    with np.errstate(all="ignore"):
        e = sm.env_eval(texels, rec[counted][:, 4:7], R) * F(scale)
        Lp[counted] = L[counted] + rec[counted][:, 0:3] * e
    last = np.zeros(state.shape, bool)
    last[..., D - 1] = True
    after_specular = np.zeros(depth.shape, bool)
    dd = depth.astype(np.int64)
    idx = np.nonzero(dd >= 2)
    after_specular[idx] = state[idx + (dd[idx] - 2,)] == V_SPECULAR
    classes = dict(
        map_open=int((is_open & (state == V_MAP)).sum()), map_occluded=int((cast & ~is_open & (state == V_MAP)).sum()),
        bsdf_open=int((is_open & (state == V_BSDF)).sum()), bsdf_occluded=int((cast & ~is_open & (state == V_BSDF)).sum()),
        no_ray_p=int((has_dir & ~positive).sum()), no_ray_fa=int((positive & (verdict == R_BLACK)).sum()), no_direction=int(((state == V_BSDF) & (verdict == R_NO_DIRECTION)).sum()),
        suppressed=int(((depth != 0) & (mark != 0)).sum()), counted_after_specular=int((counted & after_specular).sum()), specular=int((state == V_SPECULAR).sum()),
        at_max_depth=int((cast & last).sum()))
    return Result(L=L, Lp=Lp, rec=rec, c=c, cast=cast, open=is_open, nee_rays=int(cast.sum()), delta_rays=int(vtx[..., 15].sum()), classes=classes)


def render(osc, cam, spp, max_depth, seed, sample_offset, texels, tab, R=None, mix=0.5, scale=1.0, hide_background=False, walked=None):
    w = walked if walked is not None else walk(osc, cam, spp, max_depth, seed, sample_offset, mix, tab, R)
    return shade(w, texels, tab, R, scale, hide_background)


film = pm.film  # the oracle's film tiles over the samples L' after the NaN rule

# ---- the cases the two test files share (tests/test_path_nee_api.py, tests/test_gpu_path_nee.py) ---------------------------------------------------------------------
SEED = pm.SEED
DEPTHS = pm.DEPTHS
SCENE_NAMES = pm.SCENE_NAMES
MIXES = (0.25, 0.5, 15.0 / 16.0)
SCALES = (0.5, 0.0)
MAP_SIZES = (1, 7, 64)
_cache = {}


def env_of(n, turn):
    """(texels, tables, R): sky_is_model.test_map at n under the identity (None) or tests/sky_model.py's turned matrix, built once per process."""
    if ("env", n, turn) not in _cache:
        t = im.test_map(n)
        _cache["env", n, turn] = (t, im.tables(t), sm.rotation() if turn else None)
    return _cache["env", n, turn]


def matrix():
    """The parity matrix: (scene, small, depth, mix, scale, hide_background, n, turn).  Every scene x size x depth twice (once per scale), and within every scene x size
    every mix, both flags, every map size and both matrices: a covering arrangement of 64 frames, not the full product of 2304 (test_path_nee_api.py checks the cover)."""
    cases = []
    g = 0
    for which in SCENE_NAMES:
        for small in (True, False):
            for di, depth in enumerate(DEPTHS):
                for r in range(2):
                    cases.append((which, small, depth, MIXES[(2 * di + r + g) % 3], SCALES[r], bool((di + g) & 1), MAP_SIZES[(di + r + g) % 3], bool((di // 2 + r + g) & 1)))
            g += 1
    return cases


def case_id(c):
    which, small, depth, mixv, scale, hide, n, turn = c
    return "%s-%s-d%d-m%g-s%g-%s-n%d-%s" % (which, "5x3" if small else "full", depth, mixv, scale, "hide" if hide else "show", n, "turned" if turn else "identity")


def specular_scene(T):
    """Mirror and glass only: a mirror floor, the Cornell box's glass sphere and a mirror sphere beside it, under the Cornell box's lights."""
    mirror = T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.9)))
    glass = T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    quad = T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, F([[-4, 0, 2], [4, 0, 2], [4, 0, -6], [-4, 0, -6]]), F([[0, 1, 0]] * 4))
    prims = [T.GeometricPrimitive(t, mirror) for t in quad]
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.3, 0.11, -2.2]), False), 0.1, 360.0), glass))
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([-0.1, 0.25, -2.4]), False), 0.25, 360.0), mirror))
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


Y_UP = F([[1, 0, 0], [0, 0, -1], [0, 1, 0]])  # world_to_env that takes the scenes' up, +y, to the map's upper hemisphere, +z


def grey_box_scene(T):
    """All matte, no point lights: a grey box (Kd = 0.5, side 0.3) on open grey ground.  Under sky_is_model.sun_map turned by Y_UP the sun stands ahead of tests/test_gpu_sky.py's
    camera, up and to the right, and the box throws a shadow."""
    grey = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0))
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    ground = T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, F([[-40, 0, 20], [40, 0, 20], [40, 0, -40], [-40, 0, -40]]), F([[0, 1, 0]] * 4))
    x0, x1, y0, y1, z0, z1 = -0.15, 0.15, 0.0, 0.3, -2.55, -2.25
    v = F([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]])
    idx = np.uint32([1, 2, 3, 1, 3, 4, 5, 7, 6, 5, 8, 7, 1, 5, 6, 1, 6, 2, 4, 3, 7, 4, 7, 8, 1, 4, 8, 1, 8, 5, 2, 6, 7, 2, 7, 3])
    box = T.create_triangle_mesh(core, 12, idx, 8, v)
    return T.Scene([], T.BVHAccel([T.GeometricPrimitive(t, grey) for t in list(ground) + list(box)], 1))


def walked(T, which, small, max_depth, mixv, n, turn, committed=False):
    """walk() of a case, computed once per process and shared (read-only)."""
    key = ("walk", which, small, max_depth, mixv, n, turn, committed)
    if key not in _cache:
        _, tab, R = env_of(n, turn)
        w = walk(pm.scene_of(T, which, committed)[1], pm.camera(T, small, which), 1 if small else 3, max_depth, SEED, 0, mixv, tab, R)
        for a in (w.L, w.rec, w.vtx):
            a.setflags(write=False)
        _cache[key] = w
    return _cache[key]
