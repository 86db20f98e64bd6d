"""Next-event estimation of the environment map in path frames without a GPU (trhip_render_path_env_nee; docs/design/28-path-nee.md): the model of
tests/path_nee_model.py pinned to the existing models — with scale 0 its radiance is orc_render's path radiance, on a scene of mirror and glass it is tests/path_env_model.py's
frame, and its records are the path-env walk's with a mark —, the classes of vertices the GPU test's matrix must hold, the frame-wide mean against the path-env model one
depth deeper and the variance ratio on an all-matte scene under a small sun, and the interfaces: the parameter block, the refusals that need no device and their order, the
Julia file against its manifest, the Python argument checks and the calls the binding makes.  Every test asserts the facts it rests on."""
import ctypes as C
import importlib.util
import inspect
import json
import math
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import path_env_model as pm
import path_nee_model as nm
import sky_is_model as im

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPPathNEE.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_path_nee_calls.json")
INVALID = -1
# the per-sample variance of the NEE estimator (depth 3, mix 1/2) over the path-env estimator's (depth 4) on the grey box under sky_is_model.sun_map, measured on the model
# at 16 spp with the suite's seed (docs/design/28-path-nee.md "Tests"; seeds 1 and 2 gave 0.0089 and 0.0086, 8 spp 0.0076 - 0.0114)
MEASURED_VARIANCE_RATIO = 0.00817


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


# ---- the model pinned to the existing models ---------------------------------------------------------------------------------------------------------
def test_the_matrix_covers_what_the_design_lists():
    cases = nm.matrix()
    assert len(cases) == len(set(cases)) == 64
    for which in nm.SCENE_NAMES:
        for small in (True, False):
            mine = [c for c in cases if c[0] == which and c[1] == small]
            assert sorted(c[2] for c in mine) == sorted(nm.DEPTHS * 2), "every depth, once per scale"
            assert {(c[2], c[4]) for c in mine} == {(d, s) for d in nm.DEPTHS for s in nm.SCALES}
            assert {c[3] for c in mine} == set(nm.MIXES) and {c[5] for c in mine} == {False, True} and {c[6] for c in mine} == set(nm.MAP_SIZES) and {c[7] for c in mine} == {False, True}
    assert nm.MIXES == (0.25, 0.5, 15 / 16) and nm.SCALES == (0.5, 0.0) and nm.MAP_SIZES == (1, 7, 64) and nm.DEPTHS == (1, 2, 5, 8)
    for n in (7, 64):  # a bright texel in each hemisphere (the upper half of the square's diamond |x| + |y| <= 1 is z >= 0)
        t = im.test_map(n)
        c = ((np.arange(n) + 0.5) / n) * 2 - 1
        upper = (np.abs(c)[None, :] + np.abs(c)[:, None]) <= 1
        bright = t.max(axis=-1) >= 300
        assert (bright & upper).any() and (bright & ~upper).any()


def test_with_scale_zero_the_radiance_is_the_oracles_path_radiance(T, ob):
    """Pins the restated loop to path_li: every NEE contribution is +0 and no escape counts, so what is left is the point-light sum in depth order."""
    seen = set()
    for case in nm.matrix():
        which, small, depth, mixv, _, _, n, turn = case
        if (which, small, depth) in seen:
            continue
        seen.add((which, small, depth))
        _, osc = pm.scene_of(T, which)
        cam, spp = pm.camera(T, small, which), 1 if small else 3
        texels, tab, R = nm.env_of(n, turn)
        w = nm.walked(T, which, small, depth, mixv, n, turn)
        r = nm.shade(w, texels, tab, R, 0.0)
        _, ref, _ = osc.render(cam, "path", spp, depth, seed=nm.SEED, want_samples=True)
        assert not np.isnan(r.Lp).any()
        assert_bits_equal(pm.nan_rule(r.Lp), ref, nm.case_id(case))
        assert_bits_equal(r.L, w.L, "the sum in depth order is the walk's own: " + nm.case_id(case))
        assert small or r.nee_rays > 500, "the rays are cast all the same"
    assert len(seen) == 32


def test_on_mirror_and_glass_the_frame_is_the_path_env_models(T, ob):
    scene = nm.specular_scene(T)
    osc = ob.OracleScene.from_scene(scene)
    cam, texels, tab, R = pm.camera(T), *nm.env_of(7, True)
    for depth in (1, 5, 8):
        w = nm.walk(osc, cam, 3, depth, nm.SEED, 0, 0.25, tab, R)
        r = nm.shade(w, texels, tab, R, 0.5)
        ref = pm.render(osc, cam, 3, depth, nm.SEED, 0, texels, R, 0.5)
        assert r.classes["specular"] > 1000 and r.nee_rays == 0 and not r.rec[..., 7].any()
        assert_bits_equal(r.rec[..., 0:3], ref.beta, "beta")
        assert np.array_equal(r.rec[..., 3].astype(np.int32), ref.depth)
        assert_bits_equal(r.rec[..., 4:7], ref.dir, "dir")
        assert_bits_equal(r.Lp, ref.Lp, f"radiance at depth {depth}")
    assert (ref.depth >= 2).sum() > 500, "paths do bounce before they leave"


@pytest.mark.parametrize("which", nm.SCENE_NAMES)
def test_the_records_are_the_path_env_walks_with_a_mark(T, ob, which):
    """The path is trhip_render_path's in every bit, so every record is the path-env walk's; the unmarked ones — the subset that counts — in all eight floats."""
    for small in (True, False):
        for depth in (2, 8):
            w = nm.walked(T, which, small, depth, 0.5, 7, True)
            rec = pm.walked(T, which, small, depth)[1]
            unmarked = w.rec[..., 7] == 0
            assert_bits_equal(w.rec[unmarked], rec[unmarked], "the unmarked records")
            assert_bits_equal(w.rec[..., 0:7], rec[..., 0:7], "every record up to its mark")
            assert set(np.unique(w.rec[..., 7])) <= {0.0, 1.0} and not w.rec[..., 7][w.rec[..., 3] <= 1].any(), "no mark without an escape, none at depth 1"


# ---- the cases exist ---------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_holds_every_class_of_vertex(T, ob):
    """What keeps the GPU test from passing on empty ground: over its matrix the model counts vertices of every class."""
    total = {}
    for case in nm.matrix():
        which, small, depth, mixv, scale, hide, n, turn = case
        texels, tab, R = nm.env_of(n, turn)
        r = nm.shade(nm.walked(T, which, small, depth, mixv, n, turn), texels, tab, R, scale, hide)
        for k, v in r.classes.items():
            total[k] = total.get(k, 0) + v
    print("vertices over the matrix:", total)
    for k in ("map_open", "map_occluded", "bsdf_open", "bsdf_occluded", "suppressed", "counted_after_specular", "at_max_depth", "specular"):
        assert total[k] >= 100, k
    assert total["no_ray_p"] + total["no_ray_fa"] >= 100, "no ray because p or f |cos| vanishes"
    assert total["no_direction"] >= 1, "a BSDF sample without a direction"


# ---- statistics on an all-matte scene under a small sun ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grey_box(T, ob):
    """Per-sample radiance of the NEE model at depth 3 (mix 1/2) and of the path-env model at depth 4 on the grey box under sky_is_model.sun_map: (n, 3) Float64 each."""
    osc = ob.OracleScene.from_scene(nm.grey_box_scene(T))
    cam, spp = pm.camera(T), 16
    texels, (i, j) = im.sun_map()
    assert texels.shape == (64, 64, 3) and texels[j, i, 0] == 2000 and (texels == F(0.05)).sum() == 3 * (64 * 64 - 1)
    tab = im.tables(texels)
    a = nm.render(osc, cam, spp, 3, nm.SEED, 0, texels, tab, nm.Y_UP, 0.5, 1.0)
    b = pm.render(osc, cam, spp, 4, nm.SEED, 0, texels, nm.Y_UP, 1.0)
    assert a.classes["specular"] == 0 and a.delta_rays == 0 and a.nee_rays > 10000, "all matte, no point lights"
    assert not bits(b.L).any(), "everything the path-env frame shows comes from the map"
    return a.Lp.reshape(-1, 3).astype(np.float64), b.Lp.reshape(-1, 3).astype(np.float64)


def test_frame_mean_agrees_with_the_path_env_model_one_depth_deeper(grey_box):
    """NEE at vertex D stands for an escape at depth D + 1: the NEE frame at depth 3 and the path-env frame at depth 4 estimate the same integral.  The frame-wide means
    differ by at most 4 standard errors of the difference, from both estimators' per-sample variances (seed fixed: a failure is examined, not re-seeded)."""
    a, b = grey_box
    n = a.shape[0]
    assert b.shape == a.shape and np.isfinite(a).all() and np.isfinite(b).all()
    se = np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
    z = (a.mean(axis=0) - b.mean(axis=0)) / se
    print("means", a.mean(axis=0), b.mean(axis=0), "difference in standard errors:", z)
    assert (a.mean(axis=0) > 0.5).all(), "the scene is lit"
    assert np.abs(z).max() <= 4.0


def test_variance_falls_under_a_small_sun(grey_box):
    a, b = grey_box
    ratio = a.var(axis=0, ddof=1) / b.var(axis=0, ddof=1)
    print("per-sample variance, NEE over path-env:", ratio)
    assert 3 * MEASURED_VARIANCE_RATIO < 1, "three times the measured ratio still says that next-event estimation wins"
    assert ratio.max() <= 3 * MEASURED_VARIANCE_RATIO


# ---- the C interface without a device ----------------------------------------------------------------------------------------------------------------
def good_params(T, **over):
    p = T._ffi.PathNeeParams()
    assert T.lib().trhip_path_nee_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "reserved":
            for i, r in enumerate(v):
                p.reserved[i] = r
        else:
            setattr(p, k, v)
    return p


def test_parameter_block_layout_and_defaults(T):
    P = T._ffi.PathNeeParams
    assert C.sizeof(P) == 32 and [(n, P.__dict__[n].offset) for n, _ in P._fields_] == [("scale", 0), ("mix", 4), ("flags", 8), ("reserved", 12)]
    p = good_params(T)
    assert (p.scale, p.mix, p.flags, tuple(p.reserved)) == (1.0, 0.5, 0, (0, 0, 0, 0, 0))
    assert T.lib().trhip_path_nee_default_params(None) == INVALID
    header = open(os.path.join(ROOT, "include", "tracehip.h"), encoding="utf-8").read()
    body = re.search(r"typedef struct \{([^}]*)\} trhip_path_nee_params;", header).group(1)
    assert re.findall(r"(\w+) (\w+)(?:\[(\d)\])?;", body) == [("float", "scale", ""), ("float", "mix", ""), ("uint32_t", "flags", ""), ("uint32_t", "reserved", "5")]
    assert T.lib().trhip_version() == 3001


BAD_PARAMS = [
    (dict(scale=-0.5), b"scale"),
    (dict(scale=math.inf), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(flags=2), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved=(1, 0, 0, 0, 0)), b"reserved"),
    (dict(reserved=(0, 0, 0, 0, 7)), b"reserved"),
    (dict(mix=0.0), b"mix"),
    (dict(mix=1.0), b"mix"),
    (dict(mix=-0.25), b"mix"),
    (dict(mix=math.inf), b"mix"),
    (dict(mix=float("nan")), b"mix"),
]


@pytest.mark.parametrize("entry", ["trhip_render_path_env_nee", "trhip_render_path_env_nee_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    """The parameter block first — scale, flags, reserved, mix —, then trhip_render_path's refusals (the handles).  No context exists here, so every call is refused."""
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_path_env_nee" else C.c_void_p(out.ctypes.data)

    def call(p):
        return fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(p) if p is not None else None, outp, C.byref(st))

    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    # the block's own order
    assert call(good_params(T, scale=-1.0, flags=2, reserved=(1, 1, 1, 1, 1), mix=2.0)) == INVALID and b"scale" in L.trhip_last_error(None)
    assert call(good_params(T, flags=2, reserved=(1, 1, 1, 1, 1), mix=2.0)) == INVALID and b"flag" in L.trhip_last_error(None)
    assert call(good_params(T, reserved=(0, 0, 1, 0, 0), mix=2.0)) == INVALID and b"reserved" in L.trhip_last_error(None)
    assert call(None) == INVALID  # no parameter block
    assert call(good_params(T, flags=1, mix=0.25)) == INVALID and b"null argument" in L.trhip_last_error(None)  # a good block: null context and scene
    assert not out.any()


# ---- the Julia file ----------------------------------------------------------------------------------------------------------------------------------
def test_every_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPPathNEE.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_path_nee_default_params", "trhip_render_path_env_nee", "trhip_render_path_env_nee_device", "trhip_film_reduce", "trhip_env_free", "trhip_scene_free"):
        assert need in calls, need


def test_params_mirror_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipPathNeeParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    assert fields == [("scale", "Float32"), ("mix", "Float32"), ("flags", "UInt32")] + [(f"reserved{k}", "UInt32") for k in range(5)]
    assert 4 * len(fields) == C.sizeof(T._ffi.PathNeeParams) == 32


def test_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPPathNEE.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPPathNEE.jl changed: bring tests/golden/julia_shim_path_nee_calls.json in step with its ccalls"


def test_the_sky_is_file_includes_this_file_after_what_it_uses():
    """At the end of TraceHIPSkyIS.jl: after env_sampler_handle there and TraceHIPPathEnv.jl's flag and last_escapes; every existing manifest stays as it is."""
    sis = open(os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPSkyIS.jl"), encoding="utf-8").read()
    assert sis.rstrip().endswith('include("TraceHIPPathNEE.jl")') and sis.count('include("') == 1
    assert sis.index("function env_sampler_handle(") < sis.index('include("TraceHIPPathNEE.jl")')
    pe = open(os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPPathEnv.jl"), encoding="utf-8").read()
    for name in ("const TRHIP_PATH_ENV_HIDE_BACKGROUND", "function last_escapes("):
        assert 0 <= pe.index(name) < pe.index('include("TraceHIPSkyIS.jl")'), name
    for other in ("TraceHIP.jl", "TraceHIPSky.jl", "TraceHIPPathEnv.jl"):
        assert "TraceHIPPathNEE.jl" not in open(os.path.join(ROOT, "trace.jl_amd", "julia", other), encoding="utf-8").read(), other
    for name in ("julia_shim_calls.json", "julia_shim_sky_calls.json", "julia_shim_path_env_calls.json", "julia_shim_sky_is_calls.json"):
        m = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert m["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(jr.parse_ccalls(os.path.join(ROOT, m["shim"])).items())}, name


# ---- the Python class --------------------------------------------------------------------------------------------------------------------------------
def test_path_integrator_validates_env_importance(T):
    cam, smp, env = pm.camera(T, True), T.SeededSampler(1, seed=1), T.Environment.constant((1, 1, 1))
    integ = T.PathIntegrator(cam, smp, 3)
    scene = object()  # never reached: the arguments are checked before the scene is touched
    for bad in (0.0, 1.0, -0.5, 2, math.inf, float("nan"), 1.0 - 2.0 ** -30, False, "half", (0.5,)):
        with pytest.raises(T.TraceHipError, match="env_importance"):
            integ.render(scene, environment=env, env_importance=bad)
    for kw in (dict(env_scale=-1.0), dict(env_scale=math.inf)):
        with pytest.raises(T.TraceHipError, match="env_scale"):
            integ.render(scene, environment=env, env_importance=0.5, **kw)
    with pytest.raises(T.TraceHipError, match="Environment"):
        integ.render(scene, environment=np.ones((1, 1, 3)), env_importance=0.5)
    with pytest.raises(T.TraceHipError, match="needs an environment"):
        integ.render(scene, env_importance=0.5)
    with pytest.raises(T.TraceHipError, match="sample_map"):
        integ.render(scene, environment=env, env_importance=0.5, sample_map=T.SampleMap(np.ones((3, 5), np.uint32), 1))
    p = T.api.path_nee_params(env, 0.25, True, True, "test")
    assert (p.scale, p.mix, p.flags, tuple(p.reserved)) == (0.25, 0.5, T._ffi.PATH_ENV_HIDE_BACKGROUND, (0, 0, 0, 0, 0))
    assert T.api.path_nee_params(env, 1, False, 0.25, "test").mix == 0.25 and T.api.path_nee_params(env, 1, False, np.float32(0.75), "test").mix == 0.75
    sig = inspect.signature(T.PathIntegrator.render)
    assert list(sig.parameters)[-1] == "env_importance" and sig.parameters["env_importance"].default is None
    assert callable(integ.suppressed)


def test_env_importance_none_makes_todays_call_and_a_mix_the_new_one(T):
    """Behind tests/golden/make_api_calls.py's stand-in for the loaded library: without env_importance the binding calls trhip_render_path_env, argument for argument as
    before (tests/test_api_calls.py pins that record); with it, the sampler is made and trhip_render_path_env_nee is called with the 32-byte block."""
    spec = importlib.util.spec_from_file_location("make_api_calls", os.path.join(ROOT, "tests", "golden", "make_api_calls.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    ffi = T._ffi
    real_lib, real_buffer, log = ffi.lib, ffi.DeviceBuffer, []
    stub = make.StubLib(real_lib(), ffi.SIGNATURES, log)
    ffi.lib = lambda: stub
    try:
        ffi.DeviceBuffer = make.fake_buffers()
        ctx = make.FakeContext()
        scene = make.FakeScene(ctx)
        integ, env = T.PathIntegrator(make.camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4), make.environment(T)
        integ.render(scene, ctx, environment=env, env_scale=0.5, hide_background=True)
        plain = [c[0] for c in log]
        del log[:]
        integ.render(scene, ctx, environment=env, env_scale=0.5, hide_background=True, env_importance=None)
        assert [c[0] for c in log] == plain[-1:] == ["trhip_render_path_env"], "None: today's call (the environment's handle exists by now)"
        del log[:]
        integ.render(scene, ctx, environment=env, env_scale=0.5, hide_background=True, env_importance=0.25)
        assert [c[0] for c in log] == ["trhip_env_make_sampler", "trhip_render_path_env_nee"]
        del log[:]
        assert integ.render(scene, ctx, device_out=0x1000, environment=env, env_importance=True) is None
        assert [c[0] for c in log] == ["trhip_render_path_env_nee_device"], "the sampler is made once per context"
        assert integ.suppressed(scene).shape == (2, 5, 6)
        assert [c[0] for c in log][-1] == "trhip_last_escapes"
        env.close()  # behind the stand-in: its handle is none of the real library's
    finally:
        ffi.lib, ffi.DeviceBuffer = real_lib, real_buffer
