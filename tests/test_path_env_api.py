"""The environment term of path frames without a GPU (trhip_render_path_env; docs/design/26-path-env.md): the model of tests/path_env_model.py pinned to the oracle —
its base L is orc_render's per-sample path radiance bit for bit —, the properties of its records (depth-1 records are the camera rays that miss, records of a deeper frame
extend a shallower frame's), what a zero scale or a black map leaves, a furnace, the frame-wide mean against the sky model on a grey box, and the interfaces: the parameter
block, the refusals that need no device and their order, the Julia file against its manifest, the Python argument checks.  Every test asserts the facts it rests on."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import path_env_model as pm
import sky_model as sm

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPPathEnv.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_path_env_calls.json")
INVALID = -1
BETA_MAX = 18.2  # what the feasibility run of the design found as the largest throughput of an escaping path on these scenes; the model's own stays below it


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


# ---- the model against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_base_radiance_is_the_oracles_path_radiance(T, ob, which):
    """Pins the restated loop to path_li, and the layout of the scene handle between the two libraries."""
    _, osc = pm.scene_of(T, which)
    for small in (True, False):
        cam, spp = pm.camera(T, small, which), 1 if small else 3
        for depth in pm.DEPTHS:
            L, rec, _, _ = pm.walked(T, which, small, depth)
            _, ref, _ = osc.render(cam, "path", spp, depth, seed=pm.SEED, want_samples=True)
            assert not np.isnan(L).any(), "no sample is NaN on these scenes: the NaN rule changes nothing"
            assert_bits_equal(pm.nan_rule(L), ref, f"{which}, small {small}, depth {depth}")
            d = rec[..., 3]
            assert np.array_equal(d, np.floor(d)) and d.min() >= 0 and d.max() <= depth
            beta = rec[..., 0:3]
            assert np.isfinite(beta).all() and beta.min() >= 0 and beta.max() <= BETA_MAX
            assert not bits(rec[d == 0]).any(), "no escape: an all-zero record"
            assert not (np.signbit(L) & (L == 0)).any(), "L is never -0"
    d8 = pm.walked(T, which, False, 8)[1][..., 3]
    counts = [int((d8 == k).sum()) for k in range(1, 9)]
    print(which, "escapes per depth at max_depth 8:", counts, "of", d8.size)
    assert min(counts) >= 10, "every depth from 1 to 8 has escapes"
    if which in ("cornell", "unlit"):
        assert counts == [450, 943, 212, 254, 176, 169, 87, 69] and d8.size == 3627
    small8 = pm.walked(T, which, True, 8)[1][..., 3]
    assert {1, 2}.issubset(set(np.unique(small8).astype(int))) and small8.max() >= 4, "the crop holds escapes of several depths"


@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_depth_one_records_are_the_camera_rays_that_miss(T, ob, which):
    _, osc = pm.scene_of(T, which)
    for small in (True, False):
        L, rec, rays, _ = pm.walked(T, which, small, 5)
        _, prim, _, _ = osc.trace_closest(rays.reshape(-1, 8))
        miss = (prim < 0).reshape(rec.shape[:-1])
        assert 0 < miss.sum() < miss.size
        assert np.array_equal(rec[..., 3] == 1, miss)
        assert_bits_equal(rec[miss][:, 0:3], np.ones((int(miss.sum()), 3), F), "beta of a depth-1 escape")
        assert_bits_equal(rec[miss][:, 4:7], rays[miss][:, 4:7], "dir of a depth-1 escape is the camera ray's direction")
        assert not bits(rec[..., 7]).any()
        assert not bits(L[miss]).any(), "a camera ray that misses has gathered nothing"


@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_records_of_a_deeper_frame_extend_a_shallower_frames(T, ob, which):
    rec8 = pm.walked(T, which, False, 8)[1]
    for depth in (2, 5):
        rec = pm.walked(T, which, False, depth)[1]
        keep = (rec8[..., 3] >= 1) & (rec8[..., 3] <= depth)
        assert np.array_equal(keep, rec[..., 3] >= 1)
        assert_bits_equal(rec[keep], rec8[keep], f"{which}: records of depth <= {depth}")


@pytest.mark.parametrize("which", pm.SCENE_NAMES)
def test_a_zero_scale_or_a_black_map_leaves_the_base_radiance(T, ob, which):
    _, osc = pm.scene_of(T, which)
    for small in (True, False):
        w = pm.walked(T, which, small, 8)
        cam, spp = pm.camera(T, small, which), 1 if small else 3
        lit = pm.render(osc, cam, spp, 8, pm.SEED, 0, sm.random_map(7), sm.rotation(), 0.5, walked=w)
        assert (bits(lit.Lp) != bits(lit.L)).any(axis=-1).sum() >= (lit.depth > 0).sum() * 0.9, "the map does light the escapes"
        for texels, scale in ((sm.random_map(7), 0.0), (np.zeros((7, 7, 3), F), 0.5)):
            r = pm.render(osc, cam, spp, 8, pm.SEED, 0, texels, sm.rotation(), scale, walked=w)
            assert np.isfinite(r.beta).all() and not (np.signbit(r.L) & (r.L == 0)).any()
            assert_bits_equal(r.Lp, r.L, f"{which}: scale {scale}")
        hidden = pm.render(osc, cam, spp, 8, pm.SEED, 0, sm.random_map(7), sm.rotation(), 0.5, hide_background=True, walked=w)
        assert_bits_equal(hidden.Lp[lit.depth == 1], lit.L[lit.depth == 1], "hide_background: a depth-1 escape adds nothing")
        assert_bits_equal(hidden.Lp[lit.depth != 1], lit.Lp[lit.depth != 1], "hide_background: every other sample as without it")


def grey(T):
    return T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0))


def test_furnace_on_open_ground(T, ob):
    """One grey matte quad, Kd = 0.5, no lights, a constant map c: a path that leaves the ground at depth 2 brings back beta * c with beta = (Kd / pi) cos / (cos / pi) = Kd
    up to rounding.  Bound: fewer than eight Float32 roundings at 2^-24 each (the BSDF's Kd / pi, times |cos|, the pdf's cos / pi, the division, beta's product, E * scale,
    beta * c), with a twentyfold margin: 1e-5."""
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    quad = T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, F([[-40, 0, 20], [40, 0, 20], [40, 0, -40], [-40, 0, -40]]), F([[0, 1, 0]] * 4))
    scene = T.Scene([], T.BVHAccel([T.GeometricPrimitive(t, grey(T)) for t in quad], 1))
    osc = ob.OracleScene.from_scene(scene)
    c = F([0.7, 0.8, 0.9])
    r = pm.render(osc, pm.camera(T), 3, 2, pm.SEED, 0, np.broadcast_to(c, (4, 4, 3)), sm.rotation(), 1.0)
    sel = (r.depth == 2) & (r.dir[..., 1] >= 0.1)
    print("furnace: depth-2 escapes with dir.y >= 0.1:", int(sel.sum()), "of", sel.size)
    assert sel.sum() >= 1000
    err = np.abs(r.t[sel].astype(np.float64) / (0.5 * c.astype(np.float64)) - 1.0)
    print("furnace: largest |t / (0.5 c) - 1| =", err.max())
    assert err.max() <= 1e-5
    assert not bits(r.L).any(), "no lights: all radiance is the environment's"


def test_frame_mean_agrees_with_the_sky_model_on_a_grey_box(T, ob):
    """The Cornell walls without spheres, all grey Kd = 0.5, no lights: at max_depth 2 the path-env frame and the sky frame with albedo 0.5 estimate the same integral — a miss
    shows E(d), a hit brings back 0.5 E(wi) where a cosine-distributed direction leaves the box — with different random directions.  The frame-wide means differ by at most
    4 standard errors of the difference (from the two sample variances; chance failure about 2e-4 over the three channels with the seed fixed: a failure is examined, not
    re-seeded)."""
    prims, _ = T.scenes.cornell_primitives(spheres=False)
    scene = T.Scene([], T.BVHAccel([T.GeometricPrimitive(p.shape, grey(T)) for p in prims], 1))
    osc = ob.OracleScene.from_scene(scene)
    cam, spp, texels, R = pm.camera(T), 16, sm.random_map(7), sm.rotation()
    a = pm.render(osc, cam, spp, 2, pm.SEED, 0, texels, R, 1.0).Lp.reshape(-1, 3).astype(np.float64)
    n = a.shape[0]
    b = sm.render(osc, cam, spp, pm.SEED, texels, R, albedo=np.full((n, 3), 0.5, F)).L.reshape(-1, 3).astype(np.float64)
    assert b.shape == a.shape and np.isfinite(a).all() and np.isfinite(b).all()
    se = np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
    z = (a.mean(axis=0) - b.mean(axis=0)) / se
    print("means", a.mean(axis=0), b.mean(axis=0), "difference in standard errors:", z)
    assert (a.mean(axis=0) > 0.1).all(), "the box is lit"
    assert np.abs(z).max() <= 4.0


# ---- the C interface without a device ------------------------------------------------------------------------------------------------------------------
def good_params(T, **over):
    p = T._ffi.PathEnvParams()
    assert T.lib().trhip_path_env_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "reserved":
            p.reserved[0], p.reserved[1] = v
        else:
            setattr(p, k, v)
    return p


def test_parameter_block_layout_and_defaults(T):
    P = T._ffi.PathEnvParams
    assert C.sizeof(P) == 16 and [(n, P.__dict__[n].offset) for n, _ in P._fields_] == [("scale", 0), ("flags", 4), ("reserved", 8)]
    p = good_params(T)
    assert (p.scale, p.flags, tuple(p.reserved)) == (1.0, 0, (0, 0))
    assert T.lib().trhip_path_env_default_params(None) == INVALID
    assert T._ffi.PATH_ENV_HIDE_BACKGROUND == 1
    header = open(os.path.join(ROOT, "include", "tracehip.h"), encoding="utf-8").read()
    assert re.search(r"#define TRHIP_PATH_ENV_HIDE_BACKGROUND 1u", header)
    assert T.lib().trhip_version() == 3001


BAD_PARAMS = [
    (dict(scale=-0.5), b"scale"),
    (dict(scale=math.inf), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(flags=2), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved=(1, 0)), b"reserved"),
    (dict(reserved=(0, 7)), b"reserved"),
]


@pytest.mark.parametrize("entry", ["trhip_render_path_env", "trhip_render_path_env_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    """The parameter block first, then trhip_render_path's refusals (the handles).  No context exists here, so every call is refused."""
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_path_env" else C.c_void_p(out.ctypes.data)
    for over, word in BAD_PARAMS:
        assert fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(good_params(T, **over)), outp, C.byref(st)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    # the block's own order: scale before flags before reserved
    assert fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(good_params(T, scale=-1.0, flags=2, reserved=(1, 1))), outp, C.byref(st)) == INVALID and b"scale" in L.trhip_last_error(None)
    assert fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(good_params(T, flags=2, reserved=(1, 1))), outp, C.byref(st)) == INVALID and b"flag" in L.trhip_last_error(None)
    assert fn(None, None, C.byref(sn), 1, 3, 0, 0, None, None, outp, C.byref(st)) == INVALID  # no parameter block
    assert fn(None, None, C.byref(sn), 1, 3, 0, 0, None, C.byref(good_params(T, flags=1)), outp, C.byref(st)) == INVALID  # the flag is known: null context and scene
    assert b"null argument" in L.trhip_last_error(None)
    assert not out.any()


def test_records_and_relight_are_refused_without_a_frame(T):
    L = T.lib()
    out = np.zeros(8, F)
    assert L.trhip_last_escapes(None, T._ffi.fptr(out), 8) == INVALID
    for over, word in BAD_PARAMS:
        assert L.trhip_path_env_relight(None, None, C.byref(good_params(T, **over)), T._ffi.fptr(out)) == INVALID and word in L.trhip_last_error(None), over
        assert L.trhip_path_env_relight_device(None, None, C.byref(good_params(T, **over)), C.c_void_p(out.ctypes.data)) == INVALID and word in L.trhip_last_error(None), over
    assert L.trhip_path_env_relight(None, None, None, T._ffi.fptr(out)) == INVALID
    assert L.trhip_path_env_relight(None, None, C.byref(good_params(T)), T._ffi.fptr(out)) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any()


# ---- the Julia file ------------------------------------------------------------------------------------------------------------------------------
def test_every_path_env_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPPathEnv.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_path_env_default_params", "trhip_render_path_env", "trhip_render_path_env_device", "trhip_last_escapes", "trhip_path_env_relight", "trhip_film_reduce",
                 "trhip_env_free", "trhip_scene_free"):
        assert need in calls, need


def test_path_env_params_mirror_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipPathEnvParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    assert fields == [("scale", "Float32"), ("flags", "UInt32"), ("reserved0", "UInt32"), ("reserved1", "UInt32")]
    assert 4 * len(fields) == C.sizeof(T._ffi.PathEnvParams) == 16
    assert int(re.search(r"const TRHIP_PATH_ENV_HIDE_BACKGROUND = UInt32\((\d+)\)", src).group(1)) == T._ffi.PATH_ENV_HIDE_BACKGROUND


def test_path_env_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPPathEnv.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPPathEnv.jl changed: bring tests/golden/julia_shim_path_env_calls.json in step with its ccalls"


def test_the_sky_file_includes_the_path_env_file_after_what_it_uses():
    """Inside the module, at the end of TraceHIPSky.jl: after Environment and env_handle, which it uses; TraceHIP.jl's own includes and every existing manifest stay as they are."""
    sky = open(os.path.join(ROOT, "trace.jl_amd", "julia", "TraceHIPSky.jl"), encoding="utf-8").read()
    at = sky.index('include("TraceHIPPathEnv.jl")')
    for name in ("struct Environment", "function env_handle(", "struct SkyIntegrator"):
        assert 0 <= sky.index(name) < at, name
    assert sky[at:].strip() == 'include("TraceHIPPathEnv.jl")', "the include is the file's last line"
    assert 'include("TraceHIPPathEnv.jl")' not in open(jr.SHIM, encoding="utf-8").read()
    for name in ("julia_shim_calls.json", "julia_shim_sky_calls.json"):
        m = json.load(open(os.path.join(ROOT, "tests", "golden", name)))
        assert m["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(jr.parse_ccalls(os.path.join(ROOT, m["shim"])).items())}, name


# ---- the Python class --------------------------------------------------------------------------------------------------------------------------------
def test_path_integrator_validates_its_environment_arguments(T):
    cam, smp, env = pm.camera(T, True), T.SeededSampler(1, seed=1), T.Environment.constant((1, 1, 1))
    integ = T.PathIntegrator(cam, smp, 3)
    scene = object()  # never reached: the arguments are checked before the scene is touched
    for kw in (dict(env_scale=-1.0), dict(env_scale=math.inf), dict(env_scale=float("nan"))):
        with pytest.raises(T.TraceHipError, match="env_scale"):
            integ.render(scene, environment=env, **kw)
        with pytest.raises(T.TraceHipError, match="env_scale"):
            integ.relight(scene, env, **kw)
    for bad in (np.ones((1, 1, 3)), (1, 1, 1), "sky"):
        with pytest.raises(T.TraceHipError, match="Environment"):
            integ.render(scene, environment=bad)
        with pytest.raises(T.TraceHipError, match="Environment"):
            integ.relight(scene, bad)
    with pytest.raises(T.TraceHipError, match="sample_map"):
        integ.render(scene, environment=env, sample_map=T.SampleMap(np.ones((3, 5), np.uint32), 1))
    p = T.api.path_env_params(env, 0.25, True, "test")
    assert (p.scale, p.flags, tuple(p.reserved)) == (0.25, T._ffi.PATH_ENV_HIDE_BACKGROUND, (0, 0))
    assert T.api.path_env_params(env, 0, False, "test").flags == 0
    import inspect
    sig = inspect.signature(T.PathIntegrator.render)
    assert [sig.parameters[k].default for k in ("environment", "env_scale", "hide_background")] == [None, 1.0, False]
    assert callable(integ.escapes) and callable(integ.relight)
