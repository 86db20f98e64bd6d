"""Area lights in path frames without a GPU (trhip_emitters, trhip_render_path_emit; docs/design/29-path-emit.md): the model of tests/path_emit_model.py pinned to what
exists — with scale 0 its radiance is orc_render's path radiance —, the table's properties, the C++ sampler arithmetic pinned to the numpy one, the branches the GPU test's
matrix must hold, the frame-wide mean of the NEE model against the HITS_ONLY model one depth deeper and the variance ratio on an all-matte scene under a small bright quad,
and the interfaces: the parameter block, the refusals that need no device and their order, the Julia file against its manifest, the Python argument checks and the calls
the binding makes.  Every test asserts the facts it rests on."""
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
import path_emit_model as em
import path_env_model as pm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPPathEmit.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_path_emit_calls.json")
INVALID = -1
TABLE_SIZES = (1, 2, 3, 32, 288, 5000)  # 5000: above 4095, the cdf that does not fit the kernel's LDS staging
# the per-sample variance of the NEE estimator (depth 3) over the HITS_ONLY estimator's (depth 4) on the grey box under the quad, measured on the model at 16 spp with the
# suite's seed (docs/design/29-path-emit.md "Tests"; seeds 1 and 2 gave 0.00174 and 0.00215)
MEASURED_VARIANCE_RATIO = 0.00166


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


# ---- the model pinned to what exists ----------------------------------------------------------------------------------------------------------------------
def test_the_matrix_covers_what_the_design_lists():
    cases = em.matrix()
    assert len(cases) == len(set(cases)) == 56 <= 64
    for which in em.SCENE_NAMES:
        for small in (True, False):
            mine = [c for c in cases if c[0] == which and c[1] == small]
            assert sorted(c[2] for c in mine) == sorted(em.DEPTHS), "every depth"
            assert {(c[3], c[4]) for c in mine} == set(em.COMBOS), "both scales with HITS_ONLY off and on"
    assert em.DEPTHS == (1, 2, 5, 8) and set(em.COMBOS) == {(s, h) for s in (0.5, 0.0) for h in (False, True)}
    assert em.SCENE_NAMES == ("cornell_quad", "unlit_quad", "strip1", "strip4", "strip12", "materials", "zero_area")
    for depth in em.DEPTHS:  # NEE at full scale at every depth, somewhere in the matrix
        assert any(c[2] == depth and c[3] == 0.5 and not c[4] for c in cases), depth


def test_the_scenes_hold_the_emitter_sets_the_design_lists(T, ob):
    sizes = {w: em.scene_of(T, w)[3].cdf.size - 1 for w in em.SCENE_NAMES}
    assert sizes == dict(cornell_quad=2, unlit_quad=2, strip1=2, strip4=32, strip12=288, materials=3, zero_area=3)
    assert len(em.scene_of(T, "cornell_quad")[0].lights) == 1 and len(em.scene_of(T, "unlit_quad")[0].lights) == 0
    tab = em.scene_of(T, "materials")[3]
    assert len({tuple(r) for r in tab.tri[:, 12:15]}) == 2, "two emissive materials of different colours"
    assert (tab.mat_le[:, 0:3].any(axis=1)).sum() == 2
    tab = em.scene_of(T, "zero_area")[3]
    assert (tab.area64 == 0).sum() == 1 and (tab.tri[:, 3][tab.area64 == 0] == 0).all(), "the emitter material also covers a zero-area triangle, which has no probability"
    for w in em.SCENE_NAMES:
        sl = em.scene_of(T, w)[3].slots
        assert (np.diff(sl.astype(np.int64)) > 0).all(), "ascending canonical slot"


def test_with_scale_zero_the_radiance_is_the_oracles_path_radiance(T, ob):
    """Pins the restated loop to path_li: every emitted term and every emitter ray's contribution is +0, so what is left is the point-light sum in depth order.  On these
    scenes no throughput becomes non-finite (asserted), so the identity holds for every sample."""
    seen = 0
    for which in em.SCENE_NAMES:
        for small in (True, False):
            for depth in em.DEPTHS:
                for hits in (False, True):
                    _, osc, _, _ = em.scene_of(T, which)
                    cam, spp = em.camera(T, small, which), 1 if small else 3
                    r = em.rendered(T, which, small, depth, 0.0, hits)
                    _, ref, _ = osc.render(cam, "path", spp, depth, seed=em.SEED, want_samples=True)
                    assert not np.isnan(r.Lp).any()
                    assert not bits(r.Lh).any(), "Lh is +0"
                    assert_bits_equal(pm.nan_rule(r.Lp), ref, f"{which} small={small} depth={depth} hits_only={hits}")
                    assert hits or small or r.nee_rays > 500, "the rays are cast all the same"
                    assert not hits or r.nee_rays == 0
                    seen += 1
    assert seen == 7 * 2 * 4 * 2


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TABLE_SIZES)
def test_table_properties(n):
    tab = em.random_table(n)
    cdf = tab.cdf
    assert cdf.dtype == F and cdf.size == n + 1 and cdf[0] == 0 and cdf[n] == 1 and (np.diff(cdf) >= 0).all()
    assert_bits_equal(tab.tri[:, 3], cdf[1:] - cdf[:-1], "P_j")
    assert_bits_equal(tab.tri[:, 7], tab.area64.astype(F), "A_j")
    u = em.edge_triples(4096, seed=n)
    j, y, pdf = em.sample(tab, u)
    assert j.min() >= 0 and j.max() <= n - 1
    for xi in (F(0.0), em.ONE_MINUS):
        k = int(em.pick(cdf, F([xi]))[0])
        assert 0 <= k <= n - 1 and tab.tri[k, 3] > 0, (xi, k)
    weight = tab.area64 * tab.tri[:, 12:15].astype(np.float64).sum(axis=1)
    assert (weight[j] > 0).all(), "a zero-area triangle and a zero-Le material are never picked"
    assert (tab.tri[j, 3] > 0).all() and np.isfinite(pdf).all() and (pdf > 0).all()
    if n >= 32:
        assert (weight == 0).sum() >= n // 5 and len(np.unique(j)) > n // 8, "the table has weightless entries, and the triples spread over the others"
    # the picked emitter is the largest j with cdf[j] <= xi: searchsorted over the monotone table says the same
    assert np.array_equal(j, np.minimum(np.searchsorted(cdf[:n], u[:, 0], side="right") - 1, n - 1).astype(np.uint32))


@pytest.mark.parametrize("n", TABLE_SIZES)
def test_the_cpp_sampler_is_the_numpy_sampler(ob, n):
    tab = em.random_table(n)
    u = em.edge_triples(4096, seed=100 + n)
    assert {tuple(r) for r in u[:8]} == {(a, b, c) for a in (F(0), em.ONE_MINUS) for b in (F(0), em.ONE_MINUS) for c in (F(0), em.ONE_MINUS)}
    j, y, p = em.sample(tab, u)
    jc, yc, pc = em.sample_cpp(tab, u)
    assert np.array_equal(j, jc)
    assert_bits_equal(yc, y, "point")
    assert_bits_equal(pc, p, "P_j / A_j")


def test_points_lie_on_their_triangle():
    tab = em.random_table(32)
    u = em.edge_triples(4096, seed=3)
    j, y, _ = em.sample(tab, u)
    v = tab.tri[j].astype(np.float64)
    p0, p1, p2 = v[:, 0:3], v[:, 4:7], v[:, 8:11]
    m = np.stack([p1 - p0, p2 - p0], axis=-1)
    coef = np.einsum("nij,nj->ni", np.linalg.pinv(m), y.astype(np.float64) - p0)
    assert (coef > -1e-5).all() and (coef.sum(axis=1) < 1 + 1e-5).all()
    assert np.abs(np.einsum("nij,nj->ni", m, coef) + p0 - y).max() < 1e-5


# ---- the branches exist -----------------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_holds_every_listed_branch(T, ob):
    """What keeps the GPU test from passing on empty ground: over its matrix the model counts every branch of the definition."""
    total = {}
    for case in em.matrix():
        r = em.rendered(T, *case)
        for k, v in r.classes.items():
            total[k] = total.get(k, 0) + v
    print("branches over the matrix:", total)
    for k in ("counted_depth1", "counted_after_specular", "suppressed", "open", "occluded", "no_ray_fa", "no_ray_geometry", "at_max_depth", "specular", "hits_only_vertices"):
        assert total[k] >= 100, k


# ---- statistics on an all-matte scene under a small bright quad ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grey_box(T, ob):
    """Per-sample radiance of the NEE model at depth 3 and of the HITS_ONLY model at depth 4 on the grey box under the quad: (n, 3) Float64 each."""
    scene, osc, _, tab = em.scene_of(T, "grey_box")
    cam, spp = pm.camera(T), 16
    a = em.shade(em.walk(osc, cam, spp, 3, em.SEED, 0, tab, 1.0, False))
    b = em.shade(em.walk(osc, cam, spp, 4, em.SEED, 0, tab, 1.0, True))
    assert len(scene.lights) == 0 and a.classes["specular"] == 0 and a.delta_rays == 0 and b.delta_rays == 0 and a.nee_rays > 10000, "all matte, no point lights"
    assert a.classes["counted_depth1"] == 0 and b.classes["counted_depth1"] == 0, "no camera ray meets the quad"
    assert not bits(b.L).any() and not bits(a.Lh).any(), "HITS_ONLY collects through hits alone, NEE through its rays alone"
    return a.Lp.reshape(-1, 3).astype(np.float64), b.Lp.reshape(-1, 3).astype(np.float64)


def test_frame_mean_agrees_with_hits_only_one_depth_deeper(grey_box):
    """NEE at vertex D stands for a hit on an emitter at depth D + 1: the NEE frame at depth 3 and the HITS_ONLY frame at depth 4 estimate the same integral.  The
    frame-wide means differ by at most 4 standard errors of the difference, from both estimators' per-sample variances (seed fixed: a failure is examined, not re-seeded)."""
    a, b = grey_box
    n = a.shape[0]
    assert b.shape == a.shape and np.isfinite(a).all() and np.isfinite(b).all()
    se = np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
    z = (a.mean(axis=0) - b.mean(axis=0)) / se
    print("means", a.mean(axis=0), b.mean(axis=0), "difference in standard errors:", z)
    assert (a.mean(axis=0) > 0.1).all(), "the scene is lit"
    assert np.abs(z).max() <= 4.0


def test_variance_falls_under_a_small_quad(grey_box):
    a, b = grey_box
    ratio = a.var(axis=0, ddof=1) / b.var(axis=0, ddof=1)
    print("per-sample variance, NEE over HITS_ONLY:", ratio)
    assert 3 * MEASURED_VARIANCE_RATIO < 1, "three times the measured ratio still says that next-event estimation wins"
    assert ratio.max() <= 3 * MEASURED_VARIANCE_RATIO


# ---- the C interface without a device ----------------------------------------------------------------------------------------------------------------------
def good_params(T, **over):
    p = T._ffi.PathEmitParams()
    assert T.lib().trhip_path_emit_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "reserved":
            for i, r in enumerate(v):
                p.reserved[i] = r
        else:
            setattr(p, k, v)
    return p


def test_parameter_block_layout_and_defaults(T):
    P = T._ffi.PathEmitParams
    assert C.sizeof(P) == 32 and [(n, P.__dict__[n].offset) for n, _ in P._fields_] == [("scale", 0), ("flags", 4), ("reserved", 8)]
    p = good_params(T)
    assert (p.scale, p.flags, tuple(p.reserved)) == (1.0, 0, (0, 0, 0, 0, 0, 0))
    assert T.lib().trhip_path_emit_default_params(None) == INVALID
    header = open(os.path.join(ROOT, "include", "tracehip.h"), encoding="utf-8").read()
    body = re.search(r"typedef struct \{([^}]*)\} trhip_path_emit_params;", header).group(1)
    assert re.findall(r"(\w+) (\w+)(?:\[(\d)\])?;", body) == [("float", "scale", ""), ("uint32_t", "flags", ""), ("uint32_t", "reserved", "6")]
    assert re.search(r"#define TRHIP_PATH_EMIT_HITS_ONLY 1u", header) and T._ffi.PATH_EMIT_HITS_ONLY == 1
    sampler = open(os.path.join(ROOT, "include", "trace_sampler.h"), encoding="utf-8").read()
    assert re.search(r"TS_DIM_EMIT_BASE = 517\b", sampler) and em.TS_DIM_EMIT_BASE == 517 > 5 + 8 * 63, "above every vertex dimension"
    assert T.lib().trhip_version() == 3001


BAD_PARAMS = [
    (dict(scale=-0.5), b"scale"),
    (dict(scale=math.inf), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(flags=2), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved=(1, 0, 0, 0, 0, 0)), b"reserved"),
    (dict(reserved=(0, 0, 0, 0, 0, 7)), b"reserved"),
]


@pytest.mark.parametrize("entry", ["trhip_render_path_emit", "trhip_render_path_emit_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    """The parameter block first — scale, flags, reserved —, then trhip_render_path's refusals (the handles).  No context exists here, so every call is refused."""
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_path_emit" else C.c_void_p(out.ctypes.data)

    def call(p):
        return fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(p) if p is not None else None, outp, C.byref(st))

    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    # the block's own order
    assert call(good_params(T, scale=-1.0, flags=2, reserved=(1, 1, 1, 1, 1, 1))) == INVALID and b"scale" in L.trhip_last_error(None)
    assert call(good_params(T, flags=2, reserved=(1, 1, 1, 1, 1, 1))) == INVALID and b"flag" in L.trhip_last_error(None)
    assert call(good_params(T, reserved=(0, 0, 1, 0, 0, 0))) == INVALID and b"reserved" in L.trhip_last_error(None)
    assert call(None) == INVALID  # no parameter block
    assert call(good_params(T, flags=1, scale=0.25)) == INVALID and b"null argument" in L.trhip_last_error(None)  # a good block: null context and scene
    assert not out.any()


def test_emitters_entry_points_refuse_without_a_device(T):
    """trhip_emitters_create: null arguments and n_materials == 0 first, then the radiance — before any handle is looked at."""
    L = T.lib()
    ids, le, h = np.zeros(1, np.uint32), np.ones(3, F), C.c_void_p()
    fake = C.c_void_p(8)  # never dereferenced: every call below is refused before the scene is looked at

    def create(scene=fake, idp=T._ffi.u32ptr(ids), lep=T._ffi.fptr(le), n=1, out=C.byref(h)):
        return L.trhip_emitters_create(None, scene, idp, lep, n, out)

    assert create() == INVALID and b"null argument" in L.trhip_last_error(None), "a null context"
    for bad in (dict(scene=None), dict(idp=None), dict(lep=None), dict(out=None)):
        assert create(**bad) == INVALID and b"null argument" in L.trhip_last_error(None), bad
    assert not h.value
    n_tri = C.c_uint32(7)
    assert L.trhip_emitters_size(None, C.byref(n_tri)) == INVALID and n_tri.value == 7
    L.trhip_emitters_free(None)  # a no-op
    idx, pts, pdf = np.zeros(1, np.uint32), np.zeros(3, F), np.zeros(1, F)
    assert L.trhip_emitters_sample(None, None, T._ffi.fptr(le), 1, T._ffi.u32ptr(idx), T._ffi.fptr(pts), T._ffi.fptr(pdf)) == INVALID
    rec = np.zeros(4, F)
    assert L.trhip_last_emitted(None, T._ffi.fptr(rec), 4) == INVALID


# ---- the Julia file ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPPathEmit.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_emitters_create", "trhip_emitters_free", "trhip_emitters_size", "trhip_path_emit_default_params", "trhip_render_path_emit", "trhip_render_path_emit_device",
                 "trhip_last_emitted", "trhip_film_reduce", "trhip_scene_free"):
        assert need in calls, need


def test_params_mirror_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipPathEmitParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    assert fields == [("scale", "Float32"), ("flags", "UInt32")] + [(f"reserved{k}", "UInt32") for k in range(6)]
    assert 4 * len(fields) == C.sizeof(T._ffi.PathEmitParams) == 32
    assert re.search(r"const TRHIP_PATH_EMIT_HITS_ONLY = UInt32\(1\)", src)


def test_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPPathEmit.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPPathEmit.jl changed: bring tests/golden/julia_shim_path_emit_calls.json in step with its ccalls"


def test_the_path_nee_file_includes_this_file_last():
    """At the end of TraceHIPPathNEE.jl; every existing manifest stays as it is."""
    nee = open(os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPPathNEE.jl"), encoding="utf-8").read()
    assert nee.rstrip().endswith('include("TraceHIPPathEmit.jl")') and nee.count('include("') == 1
    for other in ("TraceHIP.jl", "TraceHIPSky.jl", "TraceHIPPathEnv.jl", "TraceHIPSkyIS.jl"):
        assert "TraceHIPPathEmit.jl" not in open(os.path.join(ROOT, "trace.jl_amd", "julia", other), encoding="utf-8").read(), other
    for name in ("julia_shim_calls.json", "julia_shim_sky_calls.json", "julia_shim_path_env_calls.json", "julia_shim_sky_is_calls.json", "julia_shim_path_nee_calls.json"):
        m = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert m["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(jr.parse_ccalls(os.path.join(ROOT, m["shim"])).items())}, name


# ---- the Python class --------------------------------------------------------------------------------------------------------------------------------------
class _NoHandle:
    """Stands where an Emitters would: the argument checks below end before its handle is asked for."""


def test_path_integrator_validates_the_emit_arguments(T):
    cam, smp = pm.camera(T, True), T.SeededSampler(1, seed=1)
    integ = T.PathIntegrator(cam, smp, 3)
    scene = object()  # never reached: the arguments are checked before the scene is touched
    fake = T.Emitters.__new__(T.Emitters)
    fake._h, fake.ctx = None, None
    with pytest.raises(T.TraceHipError, match="must be an Emitters"):
        integ.render(scene, emitters=_NoHandle())
    for kw in (dict(emit_scale=-1.0), dict(emit_scale=math.inf), dict(emit_scale=float("nan"))):
        with pytest.raises(T.TraceHipError, match="emit_scale"):
            integ.render(scene, emitters=fake, **kw)
    env = T.Environment.constant((1, 1, 1))
    for kw in (dict(environment=env), dict(environment=env, env_importance=0.5), dict(sample_map=T.SampleMap(np.ones((3, 5), np.uint32), 1))):
        with pytest.raises(T.TraceHipError, match="cannot be combined"):
            integ.render(scene, emitters=fake, **kw)
    p = T.api.path_emit_params(fake, 0.25, True, "test")
    assert (p.scale, p.flags, tuple(p.reserved)) == (0.25, T._ffi.PATH_EMIT_HITS_ONLY, (0,) * 6)
    assert T.api.path_emit_params(fake, 2, False, "test").flags == 0
    sig = inspect.signature(T.PathIntegrator.render)
    assert [sig.parameters[k].default for k in ("emitters", "emit_scale", "emit_hits_only")] == [None, 1.0, False]
    assert callable(integ.emitted)
    for bad in ({}, [], None, {T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0)): T.RGBSpectrum(-1.0)},
                {T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.5))): T.RGBSpectrum(math.inf)}):
        with pytest.raises(T.TraceHipError, match="Emitters"):
            T.Emitters(scene, bad)  # refused before the scene is touched


def test_emitters_none_makes_todays_call_and_a_set_the_new_one(T):
    """Behind tests/golden/make_api_calls.py's stand-in for the loaded library: without emitters the binding calls trhip_render_path, argument for argument as before
    (tests/test_api_calls.py pins that record); with a set it calls trhip_render_path_emit with the set's handle and the 32-byte block."""
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
        integ = T.PathIntegrator(make.camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4)
        integ.render(scene, ctx)
        plain = list(log)
        del log[:]
        integ.render(scene, ctx, emitters=None, emit_scale=0.5, emit_hits_only=True)
        assert [c[0] for c in log] == [c[0] for c in plain] == ["trhip_render_path"] and log == plain, "None: today's call, whatever the other two say"
        del log[:]
        fake = T.Emitters.__new__(T.Emitters)
        fake._h, fake.ctx = C.c_void_p(0x2000), ctx
        integ.render(scene, ctx, emitters=fake, emit_scale=0.5, emit_hits_only=True)
        assert [c[0] for c in log] == ["trhip_render_path_emit"]
        del log[:]
        assert integ.render(scene, ctx, device_out=0x1000, emitters=fake) is None
        assert [c[0] for c in log] == ["trhip_render_path_emit_device"]
        Lh, hits = integ.emitted(scene)
        assert Lh.shape == (2, 5, 6, 3) and hits.shape == (2, 5, 6) and hits.dtype == np.int32
        assert [c[0] for c in log][-1] == "trhip_last_emitted"
        fake._h = None  # behind the stand-in: its handle is none of the real library's
    finally:
        ffi.lib, ffi.DeviceBuffer = real_lib, real_buffer
