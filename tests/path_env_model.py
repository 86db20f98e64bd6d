"""The model of a path-env frame (trhip_render_path_env; docs/design/26-path-env.md), from the oracle alone: tests/host/path_env_oracle.cpp — the oracle's API unit, included
unchanged, plus path_li restated with the escape record — compiled here into a temporary directory with oracle/Makefile's compiler and CXXFLAGS, verbatim, and fed
OracleScene handles made by liboracle.so; the frame is finished in numpy Float32 with tests/sky_model.py's env_eval:  c = E * scale,  t = beta * c,  L' = L + t.
Nothing here calls the library under test."""
import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

import oracle_bridge as ob
import sky_model as sm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F = C.POINTER(C.c_float)
_lib = None

Result = namedtuple("Result", "L beta depth dir Lp t cam film_pos")


def makefile_flags():
    """(compiler, CXXFLAGS) as oracle/Makefile states them."""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    cxx = os.environ.get("CXX") or re.search(r"^CXX \?= (.+)$", text, re.M).group(1).strip()
    flags = re.search(r"^CXXFLAGS = (.+)$", text, re.M).group(1).split()
    for must in ("-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp"):
        assert must in flags, must
    return cxx, flags


def lib():
    global _lib
    if _lib is None:
        ob.lib()  # liboracle.so first: its scenes are what this library walks
        cxx, flags = makefile_flags()
        d = tempfile.mkdtemp(prefix="path_env_oracle_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libpath_env_oracle.so")
        subprocess.check_call([cxx] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "host", "path_env_oracle.cpp")])
        l = C.CDLL(so)
        l.path_env_walk.restype = C.c_int
        l.path_env_walk.argtypes = [C.c_void_p, C.POINTER(ob.OrcSensor), C.c_int64, C.c_int, C.c_uint64, C.c_uint32, _F, _F, _F, _F]
        l.path_env_film.restype = C.c_int
        l.path_env_film.argtypes = [C.POINTER(ob.OrcSensor), C.c_int64, C.c_uint64, C.c_uint32, _F, _F]
        _lib = l
    return _lib


def sample_shape(cam, spp):
    sb = cam.film.get_sample_bounds()
    return spp, int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1


def walk(osc, cam, spp, max_depth, seed, sample_offset=0):
    """The walk alone: raw L (spp, sb_h, sb_w, 3), the records (…, 8), the camera rays (…, 8: o, t_max, d, time) and camera_sample.film (…, 2)."""
    shape = sample_shape(cam, spp)
    L, rec, rays, fpos = np.empty(shape + (3,), F), np.empty(shape + (8,), F), np.empty(shape + (8,), F), np.empty(shape + (2,), F)
    sn = ob.make_sensor(cam)
    rc = lib().path_env_walk(osc.h, C.byref(sn), spp, max_depth, seed, sample_offset, ob.fp(L), ob.fp(rec), ob.fp(rays), ob.fp(fpos))
    assert rc == 0, "scene not committed"
    return L, rec, rays, fpos


def nan_rule(L):
    """integrators/sampler.jl:46: a sample with a NaN channel is black."""
    out = np.array(L, F)
    out[np.isnan(out).any(axis=-1)] = F(0.0)
    return out


def fold(L, rec, texels, R=None, scale=1.0, hide_background=False):
    """(L', t): c = E(dir) * scale, t = beta * c, L' = L + t where a record contributes (depth >= 1; not depth 1 under hide_background); one Float32 operation each."""
    L, rec = np.asarray(L, F), np.asarray(rec, F)
    depth = rec[..., 3]
    on = (depth != 0) & ~((depth == 1) & bool(hide_background))
    t = np.zeros_like(L)
    Lp = L.copy()
    with np.errstate(all="ignore"):
        c = sm.env_eval(texels, rec[on][:, 4:7], R) * F(scale)
        assert c.dtype == F
        t[on] = rec[on][:, 0:3] * c
        Lp[on] = L[on] + t[on]
    assert Lp.dtype == t.dtype == F
    return Lp, t


def render(osc, cam, spp, max_depth, seed, sample_offset, texels, R=None, scale=1.0, hide_background=False, walked=None):
    """The frame: base L (raw), the records (beta, depth as int32, dir), L' (raw: the NaN rule is the film pass's and trhip_last_sample_radiance's) and t, the escape's
    addend.  `walked`: walk()'s result for the same (osc, cam, spp, max_depth, seed, sample_offset), when the caller already has it."""
    L, rec, rays, fpos = walked if walked is not None else walk(osc, cam, spp, max_depth, seed, sample_offset)
    Lp, t = fold(L, rec, texels, R, scale, hide_background)
    return Result(L=L, beta=rec[..., 0:3], depth=rec[..., 3].astype(np.int32), dir=rec[..., 4:7], Lp=Lp, t=t, cam=rays, film_pos=fpos)


def film(cam, spp, seed, sample_offset, Lp):
    """The oracle's film tiles over the samples L' after the NaN rule: (H, W, 4)."""
    h, w = cam.film.size
    out = np.empty((h, w, 4), F)
    L3 = np.ascontiguousarray(nan_rule(Lp), F)
    assert L3.shape == sample_shape(cam, spp) + (3,)
    sn = ob.make_sensor(cam)
    assert lib().path_env_film(C.byref(sn), spp, seed, sample_offset, ob.fp(L3), ob.fp(out)) == 0
    return out


# ---- the cases the two test files share (tests/test_path_env_api.py, tests/test_gpu_path_env.py) ---------------------------------------------------------------------
SEED = 0x5EED0001
DEPTHS = (1, 2, 5, 8)
SCENE_NAMES = ("cornell", "mesh", "materials", "unlit")
_cache = {}


def camera(T, small=False, which=None):
    """tests/test_gpu_sky.py's two cameras: 37 x 29 under the default filter (39 x 31 x 3 = 3627 samples at 3 spp: 56 waves and a partial one), or its 5 x 3 crop under a
    filter of radius 1/2 (15 samples at 1 spp: less than a wave; the radius selects the fused record layout).  The all-materials scene's full frame is its own camera's
    (tests/shade_variants.py: 26 x 22 x 3 = 1716 samples)."""
    import test_gpu_sky as tgs
    if which == "materials" and not small:
        import shade_variants as sv
        return sv.camera(T)
    return tgs.camera(T, small)


def build_scene(T, which):
    if which == "cornell":
        return T.scenes.cornell_scene()
    if which == "mesh":
        return T.scenes.mesh_scene(16)
    if which == "unlit":  # the Cornell box without lights: everything it shows comes from the environment
        return T.Scene([], T.BVHAccel(T.scenes.cornell_primitives()[0], 1))
    if which == "materials":
        import shade_variants as sv
        return sv.build(T, tangents=False, sun="none")[0]
    raise KeyError(which)


def scene_of(T, which, committed=False):
    """(scene, oracle scene), built once per process and left alone.  committed: the oracle walks the tree the library committed (the GPU tests: needs a device); otherwise
    the oracle's own construction of the reference's tree."""
    if (which, committed) not in _cache:
        scene = build_scene(T, which)
        _cache[which, committed] = (scene, ob.OracleScene.from_scene(scene, bvh=scene.flatten().bvh() if committed else None))
    return _cache[which, committed]


def walked(T, which, small, max_depth, committed=False):
    """walk() of a case, computed once per process and shared (read-only)."""
    key = (which, small, max_depth, committed)
    if key not in _cache:
        _cache[key] = walk(scene_of(T, which, committed)[1], camera(T, small, which), 1 if small else 3, max_depth, SEED)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]
