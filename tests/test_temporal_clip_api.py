"""Variance clipping of the reprojected history (trhip_temporal_clip), the part that needs no GPU: the numpy model's own properties (tests/temporal_clip_model.py — with
gamma = +Inf it is the temporal model bit for bit; a uniform dyadic surface is relit in one frame; the synthetic case takes every branch), the parameter block's layout
(header text == ctypes mirror, 88 bytes), the default parameters, the refusals (all of the block is checked before any handle, so they are reported without a device), the
Julia file (trace.jl_amd/julia/TraceHIPTemporalClip.jl: ccalls, struct mirror, manifest, include order) and the Python class."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import denoise_model as dm
import julia_replay as jr
import temporal_clip_model as cm
import temporal_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_clip_default_params", "trhip_temporal_clip", "trhip_temporal_clip_device")
CLIP_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporalClip.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_temporal_clip_calls.json")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 5), (29, 37), (64, 64)], ids=["5x3", "37x29", "64x64"])
def test_model_with_infinite_gamma_is_the_temporal_model(size):
    """lo and hi are -+Inf, or NaN where sd = 0, and comparisons with NaN are false: nothing is clipped, and every other line is the temporal pass's."""
    h, w = size
    B, P, Hs, M = cm.synthetic(h, w, 2000 + h)
    want_out, want_hist = tm.accumulate(B, P, Hs, M, tm.SYNTHETIC_PARAMS)
    for radius in (1, 2, 3):
        tally = {}
        out, hist = cm.accumulate(B, P, Hs, M, cm.params(INF, radius), tally)
        assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(hist), bits(want_hist)), radius
        assert tally.get("clipped_low", 0) == 0 and tally.get("clipped_high", 0) == 0 and tally["inside"] > 0
    out, hist = cm.accumulate(B, P, None, None, cm.params(1.0, 3))
    want_out, want_hist = tm.accumulate(B, P, None, None, tm.SYNTHETIC_PARAMS)
    assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(hist), bits(want_hist)), "without history there is nothing to clip"


def test_model_synthetic_case_takes_every_branch():
    """At 37 x 29, for every radius, with gamma = 1: every branch of the window walk and of the clip at least once (the GPU test asserts the same on the frames it sends)."""
    for radius in (1, 2, 3):
        tally = {}
        cm.accumulate(*cm.synthetic(29, 37, 2029), cm.params(1.0, radius), tally)
        for name in cm.BRANCHES:
            assert tally.get(name, 0) >= 1, (radius, name, tally)
        assert tally["pixels_clipped"] >= 20 and tally["pixels_inside"] >= 20 and tally["blended"] >= 100, tally
    # gamma = 0 confines the history to the window's mean: every channel that is not the mean to the bit is clipped
    tally = {}
    cm.accumulate(*cm.synthetic(29, 37, 2029), cm.params(0.0, 2), tally)
    assert tally["pixels_inside"] == 0 and tally["pixels_clipped"] > 100, tally


def exact_xyz(value):
    """An XYZ triple that the pass's XYZ -> RGB turns into (value, value, value) to the bit: rgb_to_xyz of it, moved by a few ulps per component until every channel hits."""
    k = np.arange(-12, 13, dtype=np.int32)
    d = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    xyz = (dm.rgb_to_xyz(np.full(3, value, F)).view(np.int32)[None, :] + d).view(F)
    hit = (dm.xyz_to_rgb(xyz) == F(value)).all(-1)
    assert hit.any(), value
    return xyz[hit][0]


def uniform_surface(h, w, value):
    """A plane seen head-on whose positions are the pixel indices, every weight 1, and one colour that is `value` in every channel to the bit."""
    ys, xs = np.mgrid[0:h, 0:w]
    ones = np.ones((h, w), F)
    n = np.zeros((h, w, 3), F)
    n[..., 2] = 1
    p = np.stack([xs, ys, np.zeros((h, w))], -1).astype(F)
    P = dm.planes_of(n, p, np.full((h, w, 3), 0.5, F), ones, ones)
    B = np.concatenate([np.broadcast_to(exact_xyz(value), (h, w, 3)), ones[..., None]], -1).astype(F)
    return B, P, n, p


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 4.0])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_model_relights_a_uniform_dyadic_surface_in_one_frame(gamma, radius):
    """The new frame has colour 0.25 everywhere (to the bit, after the pass's own XYZ -> RGB: exact_xyz), the history colour 1.0 with N = 8 under an identity reprojection.
    Dyadic values keep the window sums exact: over cnt <= 49 positions every partial sum of m1 is k * 2^-2 and of m2 k * 2^-4, k <= 49, all Float32 numbers, so m1 = cnt / 4,
    m2 = cnt / 16, mean = 0.25 and m2 / cnt = mean * mean = 2^-4 without a rounding anywhere; var = 0, sd = 0, lo = hi = 0.25 for ANY finite gamma.  The history colour 1.0 is
    cut to 0.25 and the blend 0.25 + (0.25 - 0.25) / 8 is exactly 0.25 after ONE frame.  Unclipped it is 0.25 + 7/8 * 0.75.  (A colour that is not dyadic gives sums that
    round, a var of rounding size and an sd of its square root: the bounds then sit near the colour, not on it.)"""
    h, w = 9, 10
    B, P, n, p = uniform_surface(h, w, 0.25)
    M = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    prm = cm.Params(8.0, 0.25, 0.1, 0.5, gamma, radius)
    Hs = np.zeros((h, w, 3, 4), F)
    Hs[..., 0, :3], Hs[..., 0, 3] = F(1.0), F(8.0)
    Hs[..., 1, :3], Hs[..., 1, 3] = n, F(1.0)
    Hs[..., 2, :3] = p
    tally = {}
    out, hist = cm.accumulate(B, P, Hs, M, prm, tally)
    assert tally["blended"] == h * w and tally["clipped_high"] == 3 * h * w and tally["clipped_low"] == 0 and tally["var_floored"] == 3 * h * w
    assert tally["cut_left"] > 0 and tally["cut_right"] > 0 and tally["cut_top"] > 0 and tally["cut_bottom"] > 0, "windows of 4 to 49 positions: the sums are exact for each"
    assert np.all(hist[..., 0, :3] == F(0.25)), "exactly 0.25 after one frame"
    assert np.all(hist[..., 0, 3] == 8.0), "N' is the unclipped pass's: a clip does not shorten the history"
    assert np.array_equal(bits(out[..., :3]), bits(np.broadcast_to(dm.rgb_to_xyz(np.full(3, 0.25, F)), (h, w, 3))))
    _, plain = tm.accumulate(B, P, Hs, M, tm.Params(8.0, 0.25, 0.1, 0.5))
    assert np.all(plain[..., 0, :3] == F(0.25 + 7 / 8 * 0.75)), "unclipped, 7/8 of the old colour stays (1 + (0.25 - 1) / 8, exact)"
    _, same = cm.accumulate(B, P, Hs, M, cm.Params(8.0, 0.25, 0.1, 0.5, INF, radius))
    assert np.array_equal(bits(same), bits(plain))


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
    assert protos["trhip_temporal_clip"] == protos["trhip_temporal"] and protos["trhip_temporal_clip_device"] == protos["trhip_temporal_device"]
    assert T.lib().trhip_version() == 3001, "nothing existing moved: the ABI number stays"


def test_params_mirror_matches_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_temporal_clip_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == [("base", "trhip_temporal_params"), ("clip_gamma", "float"), ("clip_radius", "uint32_t"), ("flags", "uint32_t"), ("reserved", "uint32_t")]
    S = T._ffi.TemporalClipParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32, "trhip_temporal_params": T._ffi.TemporalParams}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(S._fields_)
    assert C.sizeof(S) == 88 and C.sizeof(T._ffi.TemporalParams) == 72
    assert [getattr(S, n).offset for n, _ in fields] == [0, 72, 76, 80, 84]


def good_params(T, **over):
    p = T._ffi.TemporalClipParams()
    assert T.lib().trhip_temporal_clip_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "matrix_entry":
            p.base.prev_world_to_pixel[v[0]] = v[1]
        elif k.startswith("base_"):
            setattr(p.base, k[5:], v)
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.TemporalClipParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_temporal_clip_default_params(C.byref(p)) == 0
    base = T._ffi.TemporalParams()
    assert T.lib().trhip_temporal_default_params(C.byref(base)) == 0
    assert bytes(p.base) == bytes(base), "base is what trhip_temporal_default_params fills"
    assert p.clip_radius in (1, 2, 3) and p.clip_gamma >= 0.0 and (p.flags, p.reserved) == (0, 0)
    assert T.lib().trhip_temporal_clip_default_params(None) == INVALID


# trhip_temporal's refusals on base, in its order, then the new fields
BAD_PARAMS = [(dict(matrix_entry=(0, float("nan"))), b"prev_world_to_pixel"), (dict(matrix_entry=(11, INF)), b"prev_world_to_pixel"),
              (dict(base_max_history=0.5), b"max_history"), (dict(base_max_history=INF), b"max_history"), (dict(base_max_history=float("nan")), b"max_history"),
              (dict(base_flags=1), b"trhip_temporal: unknown flag"), (dict(base_reserved=1), b"trhip_temporal: reserved"),
              (dict(base_min_coverage=-0.1), b"min_coverage"), (dict(base_min_coverage=1.5), b"min_coverage"), (dict(base_min_coverage=float("nan")), b"min_coverage"),
              (dict(clip_gamma=float("nan")), b"clip_gamma"), (dict(clip_gamma=-1.0), b"clip_gamma"), (dict(clip_gamma=-INF), b"clip_gamma"),
              (dict(clip_radius=0), b"clip_radius"), (dict(clip_radius=4), b"clip_radius"), (dict(clip_radius=0xFFFFFFFF), b"clip_radius"),
              (dict(flags=1), b"trhip_temporal_clip: unknown flag"), (dict(reserved=7), b"trhip_temporal_clip: reserved"),
              # the order: base before the new fields, and those in the order of the block
              (dict(base_reserved=1, clip_gamma=-1.0), b"trhip_temporal: reserved"), (dict(clip_gamma=-1.0, clip_radius=9, flags=1), b"clip_gamma"),
              (dict(clip_radius=9, flags=1), b"clip_radius"), (dict(flags=1, reserved=1), b"unknown flag")]
for _name in ("sigma_normal", "sigma_plane"):
    BAD_PARAMS += [({"base_" + _name: v}, _name.encode()) for v in (0.0, -1.0, INF, float("nan"))]


@pytest.mark.parametrize("entry", ["trhip_temporal_clip", "trhip_temporal_clip_device"])
def test_invalid_parameter_blocks_are_refused_without_a_device(T, entry):
    """No context exists here, so every call is refused; all of the parameter block is checked first, and the message (kept for trhip_last_error(NULL)) names the field."""
    fn, L = getattr(T.lib(), entry), T.lib()
    film, planes, out, out_h = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F)
    ptr = (lambda a: T._ffi.fptr(a)) if entry == "trhip_temporal_clip" else (lambda a: C.c_void_p(a.ctypes.data))
    for over, word in BAD_PARAMS:
        assert fn(None, ptr(film), ptr(planes), None, 2, 2, C.byref(good_params(T, **over)), ptr(out), ptr(out_h), None) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    assert fn(None, ptr(film), ptr(planes), None, 2, 2, None, ptr(out), ptr(out_h), None) == INVALID  # no parameter block
    for over in (dict(), dict(clip_gamma=0.0), dict(clip_gamma=INF), dict(clip_radius=1), dict(clip_radius=2), dict(clip_radius=3)):  # valid blocks: only the context is missing
        assert fn(None, ptr(film), ptr(planes), None, 2, 2, C.byref(good_params(T, **over)), ptr(out), ptr(out_h), None) == INVALID, over
        assert b"null argument" in L.trhip_last_error(None), over
    assert not out.any() and not out_h.any()


# ---- the Julia file --------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_clip_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(CLIP_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPTemporalClip.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_temporal_clip", "trhip_temporal_clip_default_params"]


def test_julia_clip_params_mirror_the_header(T):
    """Julia has no inline field of a mutable struct type, so the file writes `base` out field by field (its flags and reserved as base_flags, base_reserved)."""
    src = open(CLIP_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalClipParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    ct = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{12,Float32}": C.c_float * 12}
    S = T._ffi.TemporalClipParams
    flat = [("base_" + n if n in ("flags", "reserved") else n, c, S.base.offset + getattr(T._ffi.TemporalParams, n).offset) for n, c in T._ffi.TemporalParams._fields_]
    flat += [(n, c, getattr(S, n).offset) for n, c in S._fields_[1:]]
    assert [n for n, _ in fields] == [n for n, _, _ in flat]
    assert [C.sizeof(ct[t]) for _, t in fields] == [C.sizeof(c) for _, c, _ in flat]
    offsets = np.cumsum([0] + [C.sizeof(ct[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [o for _, _, o in flat] and offsets[-1] == C.sizeof(S) == 88


def test_clip_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(CLIP_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPTemporalClip.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPTemporalClip.jl changed: bring tests/golden/julia_shim_temporal_clip_calls.json in step with its ccalls"


def test_the_shim_includes_the_clip_file_after_the_temporal_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPTemporalClip.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPTemporal.jl")') < at < src.rindex("end # module")
    temporal = open(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporal.jl"), encoding="utf-8").read()
    for name in ("mutable struct TrhipTemporalParams", "struct TemporalAccumulator", "function temporal_params("):  # what the clip file uses of the file before it
        assert name in temporal, name


# ---- Python ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_classes(T):
    t = T.TemporalAccumulator()
    assert type(t.params) is T._ffi.TemporalParams and C.sizeof(t.params) == 72 and t.clip_params is None, "no clip argument: today's block, today's entry points"
    d = good_params(T)
    t = T.TemporalAccumulator(clip_gamma=2.0)
    assert isinstance(t.clip_params, T._ffi.TemporalClipParams) and (t.clip_params.clip_gamma, t.clip_params.clip_radius) == (2.0, d.clip_radius)
    t = T.TemporalAccumulator(clip_radius=1)
    assert (t.clip_params.clip_gamma, t.clip_params.clip_radius) == (d.clip_gamma, 1)
    t = T.TemporalAccumulator(max_history=16, sigma_normal=0.02, clip_gamma=INF, clip_radius=2)
    assert (t.params.max_history, t.params.sigma_normal) == (16.0, F(0.02)), "params stays the base block"
    cam_matrix = np.arange(12, dtype=F).reshape(3, 4)
    cp = t._clip_params_for(cam_matrix)
    assert C.sizeof(cp) == 88 and list(cp.base.prev_world_to_pixel) == list(range(12))
    assert (cp.base.max_history, cp.base.sigma_normal, cp.clip_gamma, cp.clip_radius, cp.flags, cp.reserved) == (16.0, F(0.02), INF, 2, 0, 0)
    assert list(t.clip_params.base.prev_world_to_pixel) == [0.0] * 12, "the accumulator's own block keeps the placeholder matrix"
    with pytest.raises(T.TraceHipError):
        T.TemporalAccumulator(clip_radius=1.5)
    s = T.PreviewSession(T.scenes.cornell_scene(), T.SeededSampler(2, seed=3), 3, temporal=T.TemporalAccumulator(clip_gamma=1.0))
    assert s.temporal.clip_params is not None
    s.scene = s.scene.with_lights(s.scene.lights)
    s.reset()
    s.close()
