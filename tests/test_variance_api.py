"""The variance passes (trhip_temporal_moments, trhip_denoise_var), the part that needs no GPU: the numpy model's own properties (tests/variance_model.py — unit variance and
one iteration is the denoiser model bit for bit; a surface of one dyadic luminance has variance exactly 0; the synthetic cases take every branch; colours stay finite whatever
the variance plane holds), the parameter blocks' layouts (header text == ctypes mirror, 88 and 48 bytes), the default parameters, the refusals in their stated order (all of a
block is checked before any handle, so they are reported without a device) and the Python classes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_model as dm
import julia_replay as jr
import temporal_model as tm
import variance_model as vm
from test_temporal_clip_api import uniform_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF, NAN = float("inf"), float("nan")
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_moments_default_params", "trhip_temporal_moments", "trhip_temporal_moments_device", "trhip_denoise_var_default_params", "trhip_denoise_var",
                "trhip_denoise_var_device")
MOMENTS_BRANCHES = ("temporal", "spatial", "short", "colour_restart", "moments_restart", "no_taps", "window_cut", "window_rejected", "spatial_floored")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False])
def test_model_unit_variance_and_one_iteration_is_the_denoiser_model(demodulate):
    """gs and gw add the same weights in the same order, so gv = 1 exactly, sd = 1, sig = 3.5 * 1 + 0.5 = 4: the colour weights are the plain filter's at sigma_colour = 4."""
    B, P, _ = dm.synthetic(29, 37, 11)
    out, var = vm.denoise(B, P, np.ones((29, 37), F), vm.VarParams(3.5, 0.25, 0.1, iterations=1, demodulate=demodulate, var_eps=0.5))
    want = dm.denoise(B, P, dm.Params(4.0, 0.25, 0.1, iterations=1, demodulate=demodulate))
    assert np.array_equal(bits(out), bits(want))
    surface = dm.surface_mask(B, P, dm.Params(4.0, 0.25, 0.1, demodulate=demodulate))
    assert np.all(var[surface] > 0) and np.all(var[surface] <= 1) and not var[~surface].any(), "sum w^2 / (sum w)^2 of a unit variance lies in (0, 1]"


@pytest.mark.parametrize("kind", ["zero", "one", "random", "poisoned"])
def test_model_colours_are_finite_whatever_the_variance_plane_holds(kind):
    B, P, poisoned = dm.synthetic(29, 37, 12)
    prm = vm.VarParams(4.0, 0.25, 0.1, iterations=3, var_eps=2.0 ** -6)
    tally = {}
    out, var = vm.denoise(B, P, vm.synthetic_variance(29, 37, 12, kind), prm, tally)
    surface = dm.surface_mask(B, P, prm)
    assert np.isfinite(out[surface]).all() and not np.isnan(var).any() and np.all(var >= 0) and not var[~surface].any()
    assert np.array_equal(bits(out[~surface]), bits(B[~surface])) and np.array_equal(bits(out[..., 3]), bits(B[..., 3]))
    if kind == "poisoned":
        assert tally["inf_sigma"] > 0 and tally["nan_variance"] > 0, tally
    else:
        assert np.isfinite(var).all()
    if kind == "zero":
        assert not var.any(), "a variance of 0 stays 0: sig = var_eps"
    assert tally["colour"][0] > 0 and tally["colour"][1] > 0, tally


def test_model_moments_keep_the_temporal_models_colour_and_take_every_branch():
    for demodulate in (True, False):
        B, P, Hs, Ms, M = vm.synthetic_moments(29, 37, 2029)
        tally = {}
        out, hist, mom, var = vm.accumulate(B, P, Hs, Ms, M, vm.moments_params(demodulate), tally)
        want_out, want_hist = tm.accumulate(B, P, Hs, M, tm.SYNTHETIC_PARAMS)
        assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(hist), bits(want_hist))
        for name in MOMENTS_BRANCHES:
            assert tally.get(name, 0) >= 1, (name, tally)
        surface = hist[..., 1, 3] == 1
        assert np.isfinite(var).all() and np.all(var >= 0) and np.isfinite(mom).all() and not var[~surface].any() and not mom[~surface].any()
        # without history every surface pixel restarts: m1 = Yd, m2 = Yd * Yd, the spatial estimate, N' = 1
        out0, hist0, mom0, var0 = vm.accumulate(B, P, None, None, None, vm.moments_params(demodulate), t0 := {})
        assert t0["spatial"] == surface.sum() and t0.get("temporal", 0) == 0
        assert np.array_equal(bits(mom0[surface, 1]), bits(mom0[surface, 0] * mom0[surface, 0]))


def test_model_dyadic_surface_has_variance_zero():
    """One luminance, 0.25 to the bit in every channel (demodulation off): window sums of k * 2^-2 and k * 2^-4, k <= 49, are exact, mean = 0.25, S2 / cnt = mean^2: vs = 0.
    With a history of the same moments (0.25, 0.0625) the blend is exact too: vt = 0, for histories below and above spatial_below alike."""
    h, w = 9, 10
    B, P, n, p = uniform_surface(h, w, 0.25)
    M = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    prm = vm.MomentsParams(8.0, 0.25, 0.1, 0.5, 1.0 / 64.0, 4.0, False)
    out, hist, mom, var = vm.accumulate(B, P, None, None, None, prm)
    assert not var.any() and np.all(mom[..., 0] == F(0.25)) and np.all(mom[..., 1] == F(0.0625))
    hist[..., 0, 3] = np.where(np.arange(w)[None, :] % 2 == 0, F(1.0), F(6.0))  # N' = 2 (spatial) and 7 (temporal) side by side
    tally = {}
    out, hist2, mom2, var2 = vm.accumulate(B, P, hist, mom, M, prm, tally)
    assert tally["temporal"] > 0 and tally["short"] > 0 and not var2.any()
    assert np.array_equal(bits(mom2), bits(mom))


# ---- the C interface ---------------------------------------------------------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "tracehip.h")).read()


def test_entry_points_are_exported_with_the_headers_signatures(T):
    protos = jr.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, f"include/tracehip.h does not declare {name}"
        assert getattr(T.lib(), name) is not None
        ret, args = T._ffi.SIGNATURES[name]
        c_ret, c_args = jr.ctypes_sig(protos[name])
        assert ret is c_ret and len(args) == len(c_args), name
        for k, (a, c) in enumerate(zip(args, c_args)):
            if c is C.c_void_p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, k, a)
            else:
                assert a is c, (name, k, a, c)
    assert T.lib().trhip_version() == 3001, "nothing existing moved: the ABI number stays"


def header_fields(name):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s\s*;" % name, src).group(1)
    return [(m.group(2), m.group(1), m.group(3)) for m in re.finditer(r"(\w+)\s+(\w+)\s*(\[\d+\])?\s*;", body)]


def test_params_mirrors_match_the_header(T):
    assert header_fields("trhip_temporal_moments_params") == [("base", "trhip_temporal_params", None), ("albedo_floor", "float", None), ("spatial_below", "float", None),
                                                              ("flags", "uint32_t", None), ("reserved", "uint32_t", None)]
    S = T._ffi.TemporalMomentsParams
    assert list(S._fields_) == [("base", T._ffi.TemporalParams), ("albedo_floor", C.c_float), ("spatial_below", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]
    assert C.sizeof(S) == 88 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 72, 76, 80, 84]
    assert header_fields("trhip_denoise_var_params") == [("base", "trhip_denoise_params", None), ("var_eps", "float", None), ("flags", "uint32_t", None), ("reserved", "uint32_t", "[2]")]
    S = T._ffi.DenoiseVarParams
    assert [n for n, _ in S._fields_] == ["base", "var_eps", "flags", "reserved"] and S._fields_[0][1] is T._ffi.DenoiseParams and C.sizeof(S._fields_[3][1]) == 8
    assert C.sizeof(S) == 48 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 32, 36, 40]


def test_default_params_need_no_context(T):
    L = T.lib()
    p = T._ffi.TemporalMomentsParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert L.trhip_temporal_moments_default_params(C.byref(p)) == 0
    base = T._ffi.TemporalParams()
    assert L.trhip_temporal_default_params(C.byref(base)) == 0
    assert bytes(p.base) == bytes(base), "base is what trhip_temporal_default_params fills"
    d = T._ffi.DenoiseParams()
    assert L.trhip_denoise_default_params(C.byref(d)) == 0
    assert p.albedo_floor == d.albedo_floor and p.spatial_below >= 1.0 and (p.flags, p.reserved) == (T._ffi.DENOISE_DEMODULATE, 0)
    assert L.trhip_temporal_moments_default_params(None) == INVALID
    v = T._ffi.DenoiseVarParams()
    C.memset(C.byref(v), 0xFF, C.sizeof(v))
    assert L.trhip_denoise_var_default_params(C.byref(v)) == 0
    d.sigma_colour = v.base.sigma_colour
    assert bytes(v.base) == bytes(d), "base is trhip_denoise_default_params' but for sigma_colour, which has another meaning here"
    assert v.base.sigma_colour > 0 and v.var_eps > 0 and v.flags == 0 and list(v.reserved) == [0, 0]
    assert L.trhip_denoise_var_default_params(None) == INVALID


def good_moments(T, **over):
    p = T._ffi.TemporalMomentsParams()
    assert T.lib().trhip_temporal_moments_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "matrix_entry":
            p.base.prev_world_to_pixel[v[0]] = v[1]
        elif k.startswith("base_"):
            setattr(p.base, k[5:], v)
        else:
            setattr(p, k, v)
    return p


# trhip_temporal's refusals on base, in its order, then albedo_floor, spatial_below, flags, reserved
BAD_MOMENTS = [(dict(matrix_entry=(0, NAN)), b"prev_world_to_pixel"), (dict(base_max_history=0.5), b"max_history"), (dict(base_flags=1), b"trhip_temporal: unknown flag"),
               (dict(base_sigma_normal=0.0), b"sigma_normal"), (dict(base_sigma_plane=NAN), b"sigma_plane"), (dict(base_min_coverage=1.5), b"min_coverage"),
               (dict(base_reserved=1), b"trhip_temporal: reserved"),
               (dict(albedo_floor=0.0), b"albedo_floor"), (dict(albedo_floor=INF), b"albedo_floor"), (dict(albedo_floor=NAN), b"albedo_floor"), (dict(albedo_floor=-1.0), b"albedo_floor"),
               (dict(spatial_below=0.5), b"spatial_below"), (dict(spatial_below=INF), b"spatial_below"), (dict(spatial_below=NAN), b"spatial_below"),
               (dict(flags=2), b"trhip_temporal_moments: unknown flag"), (dict(flags=0x80000001), b"trhip_temporal_moments: unknown flag"), (dict(reserved=7), b"trhip_temporal_moments: reserved"),
               # the order
               (dict(base_reserved=1, albedo_floor=0.0), b"trhip_temporal: reserved"), (dict(albedo_floor=0.0, spatial_below=0.0, flags=2, reserved=1), b"albedo_floor"),
               (dict(spatial_below=0.0, flags=2, reserved=1), b"spatial_below"), (dict(flags=2, reserved=1), b"unknown flag")]


@pytest.mark.parametrize("entry", ["trhip_temporal_moments", "trhip_temporal_moments_device"])
def test_invalid_moments_blocks_are_refused_without_a_device(T, entry):
    """No context exists here, so every call is refused; all of the parameter block is checked first, and the message (kept for trhip_last_error(NULL)) names the field."""
    fn, L = getattr(T.lib(), entry), T.lib()
    film, planes, out, out_h, out_m, out_v = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2, 2), F), np.zeros((2, 2), F)
    ptr = (lambda a: T._ffi.fptr(a)) if entry == "trhip_temporal_moments" else (lambda a: C.c_void_p(a.ctypes.data))
    call = lambda prm: fn(None, ptr(film), ptr(planes), None, None, 2, 2, prm, ptr(out), ptr(out_h), ptr(out_m), ptr(out_v), None)  # noqa: E731
    for over, word in BAD_MOMENTS:
        assert call(C.byref(good_moments(T, **over))) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    assert call(None) == INVALID
    for over in (dict(), dict(flags=0), dict(spatial_below=1.0), dict(spatial_below=64.0)):  # valid blocks: only the context is missing
        assert call(C.byref(good_moments(T, **over))) == INVALID, over
        assert b"null argument" in L.trhip_last_error(None), over
    assert not out.any() and not out_h.any() and not out_m.any() and not out_v.any()


def good_var(T, **over):
    p = T._ffi.DenoiseVarParams()
    assert T.lib().trhip_denoise_var_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "reserved":
            p.reserved[v[0]] = v[1]
        elif k.startswith("base_"):
            setattr(p.base, k[5:], v)
        else:
            setattr(p, k, v)
    return p


# trhip_denoise's refusals on base, in its order, then var_eps, flags, reserved
BAD_VAR = [(dict(base_iterations=7), b"iterations"), (dict(base_flags=2), b"trhip_denoise: unknown flag"), (dict(base_sigma_colour=0.0), b"sigma_colour"),
           (dict(base_sigma_colour=INF), b"sigma_colour"), (dict(base_sigma_normal=NAN), b"sigma_normal"), (dict(base_sigma_plane=-1.0), b"sigma_plane"),
           (dict(base_albedo_floor=0.0), b"albedo_floor"), (dict(base_min_coverage=2.0), b"min_coverage"), (dict(base_reserved=1), b"trhip_denoise: reserved"),
           (dict(var_eps=0.0), b"var_eps"), (dict(var_eps=-1.0), b"var_eps"), (dict(var_eps=INF), b"var_eps"), (dict(var_eps=NAN), b"var_eps"),
           (dict(flags=1), b"trhip_denoise_var: unknown flag"), (dict(reserved=(0, 1)), b"trhip_denoise_var: reserved"), (dict(reserved=(1, 1)), b"trhip_denoise_var: reserved"),
           (dict(base_reserved=1, var_eps=0.0), b"trhip_denoise: reserved"), (dict(var_eps=0.0, flags=1, reserved=(0, 1)), b"var_eps"), (dict(flags=1, reserved=(0, 1)), b"unknown flag")]


@pytest.mark.parametrize("entry", ["trhip_denoise_var", "trhip_denoise_var_device"])
def test_invalid_var_blocks_are_refused_without_a_device(T, entry):
    fn, L = getattr(T.lib(), entry), T.lib()
    film, planes, var, out, out_v = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2), F), np.zeros((2, 2, 4), F), np.zeros((2, 2), F)
    ptr = (lambda a: T._ffi.fptr(a)) if entry == "trhip_denoise_var" else (lambda a: C.c_void_p(a.ctypes.data))
    call = lambda prm: fn(None, ptr(film), ptr(planes), ptr(var), 2, 2, prm, ptr(out), ptr(out_v), None)  # noqa: E731
    for over, word in BAD_VAR:
        assert call(C.byref(good_var(T, **over))) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    assert call(None) == INVALID
    for over in (dict(), dict(base_iterations=0), dict(base_flags=0), dict(var_eps=2.0 ** -12)):
        assert call(C.byref(good_var(T, **over))) == INVALID, over
        assert b"null argument" in L.trhip_last_error(None), over
    assert not out.any() and not out_v.any()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_classes(T):
    t = T.TemporalAccumulator()
    assert type(t.params) is T._ffi.TemporalParams and t.clip_params is None and t.moments_params is None, "no new argument: today's block, today's entry points"
    d = good_moments(T)
    t = T.TemporalAccumulator(moments=True)
    assert isinstance(t.moments_params, T._ffi.TemporalMomentsParams) and t.clip_params is None
    assert (t.moments_params.spatial_below, t.moments_params.albedo_floor, t.moments_params.flags) == (d.spatial_below, d.albedo_floor, 1)
    t = T.TemporalAccumulator(max_history=16, sigma_normal=0.02, moments=True, spatial_below=2, demodulate=False, albedo_floor=0.25)
    assert (t.params.max_history, t.params.sigma_normal) == (16.0, F(0.02)), "params stays the base block"
    mp = t._moments_params_for(np.arange(12, dtype=F).reshape(3, 4))
    assert C.sizeof(mp) == 88 and list(mp.base.prev_world_to_pixel) == list(range(12))
    assert (mp.base.max_history, mp.base.sigma_normal, mp.spatial_below, mp.albedo_floor, mp.flags, mp.reserved) == (16.0, F(0.02), 2.0, 0.25, 0, 0)
    assert list(t.moments_params.base.prev_world_to_pixel) == [0.0] * 12, "the accumulator's own block keeps the placeholder matrix"
    for kw in (dict(clip_gamma=1.0), dict(clip_radius=2), dict(clip_gamma=INF, clip_radius=1)):
        with pytest.raises(T.TraceHipError, match="moments=True cannot be combined"):
            T.TemporalAccumulator(moments=True, **kw)
    with pytest.raises(T.TraceHipError, match="belong to moments=True"):
        T.TemporalAccumulator(spatial_below=2.0)
    B, P = np.zeros((3, 5, 4), F), np.zeros((3, 5, 3, 4), F)
    with pytest.raises(T.TraceHipError, match="needs TemporalAccumulator\\(moments=True\\)"):
        T.TemporalAccumulator().accumulate_moments(B, P, None, None, None)
    t = T.TemporalAccumulator(moments=True)
    for args in ((B[..., :3], P, None, None), (B, P[:2], None, None), (B, P, P, None), (B, P, None, np.zeros((3, 5, 2), F)), (B, P, P[:2], np.zeros((3, 5, 2), F)),
                 (B, P, P, np.zeros((3, 5), F))):
        with pytest.raises(T.TraceHipError, match="accumulate_moments: "):
            t.accumulate_moments(*args, None)
    dn = T.Denoiser(iterations=3, sigma_colour=2.0, demodulate=False)
    v = good_var(T)
    assert (dn.variance_sigma, dn.var_eps) == (v.base.sigma_colour, v.var_eps) and dn.params.sigma_colour == 2.0
    vp = T.Denoiser(iterations=3, sigma_colour=2.0, demodulate=False, variance_sigma=1.5, var_eps=0.125)._var_params()
    assert (vp.base.iterations, vp.base.flags, vp.base.sigma_colour, vp.var_eps, vp.flags, list(vp.reserved)) == (3, 0, 1.5, 0.125, 0, [0, 0])
    for args in ((B[..., :3], P, np.zeros((3, 5), F)), (B, P, np.zeros((5, 3), F)), (B, P[:2], np.zeros((3, 5), F))):
        with pytest.raises(T.TraceHipError, match="denoise_variance: "):
            dn.denoise_variance(*args)
    scene = T.scenes.cornell_scene()
    s = T.PreviewSession(scene, T.SeededSampler(2, seed=3), 3, variance_guided=True)
    assert s.temporal.moments_params is not None and s.variance_guided
    s.close()
    with pytest.raises(T.TraceHipError, match="needs a TemporalAccumulator\\(moments=True\\)"):
        T.PreviewSession(scene, T.SeededSampler(2, seed=3), 3, temporal=T.TemporalAccumulator(), variance_guided=True)
    s = T.PreviewSession(scene, T.SeededSampler(2, seed=3), 3)
    assert not s.variance_guided and s.temporal.moments_params is None
    s.close()
