"""trace.jl_amd/julia/TraceHIPAdaptive.jl (the adaptive-sampling part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_direct_split.py checks
TraceHIPDirectSplit.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the manifest tests/golden/julia_shim_adaptive_calls.json is the one the
source produces, TraceHIP.jl includes the file inside its module after TraceHIPDirectSplit.jl, the parameter block is the header's, and the shim's own signatures, replayed
through ctypes with a NULL context, reach the library's argument checks."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPAdaptive.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_adaptive_calls.json")
F = np.float32


def test_every_adaptive_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPAdaptive.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_film_sum", "trhip_last_sample_stats", "trhip_render_path", "trhip_render_path_map", "trhip_sample_map", "trhip_sample_map_default_params",
                             "trhip_scene_free"]
    # trhip_render_path's arguments with the map and max_spp where spp stood
    path, mapped = calls["trhip_render_path"][0][1], calls["trhip_render_path_map"][0][1]
    assert mapped == path[:3] + ["ptr:u32", "u32"] + path[4:]


def test_adaptive_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPAdaptive.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPAdaptive.jl changed: bring tests/golden/julia_shim_adaptive_calls.json in step with its ccalls"


def test_the_shim_includes_the_adaptive_file_after_the_direct_split_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPAdaptive.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPDirectSplit.jl")') < at < src.rindex("end # module")
    assert all(m.start() <= at for m in re.finditer(r'^include\("TraceHIP\w+\.jl"\)', src, flags=re.M)), "after the last existing include"
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}  # the include adds no ccall to TraceHIP.jl itself


def test_the_julia_parameter_block_is_the_headers(T):
    src = open(SHIM, encoding="utf-8").read()
    block = src[src.index("mutable struct TrhipSampleMapParams"):]
    block = block[:block.index("\nend")]
    fields = re.findall(r"^\s+(\w+)::(\w+)$", block, flags=re.M)
    assert fields == [("tau", "Float32"), ("eps", "Float32"), ("pilot", "UInt32"), ("max_extra", "UInt32"), ("flags", "UInt32"), ("reserved", "UInt32")]
    assert [f for f, _ in T._ffi.SampleMapParams._fields_] == [f for f, _ in fields] and C.sizeof(T._ffi.SampleMapParams) == 24
    # the integrator fills what the Python one fills: the pilot count from the sampler, the rest only when given
    fill = src[src.index("function sample_map_params("):]
    fill = fill[:fill.index("\nend")]
    assert "p.pilot = i.sampler.samples_per_pixel" in fill
    for f in ("tau", "max_extra", "eps"):
        assert f"i.{f} === nothing || (p.{f} = i.{f})" in fill
    call = src[src.index("function (i::AdaptivePathIntegrator)("):]
    assert "sample_offset = n0" in call and "total > 0" in call and "film_sum(pilot, extra, w, h)" in call


def test_the_shims_signatures_replayed_through_ctypes_reach_the_argument_checks(T):
    calls = jr.parse_ccalls(SHIM)
    L = C.CDLL(T.lib()._name)
    fns = {}
    for name in ("trhip_render_path_map", "trhip_last_sample_stats", "trhip_sample_map", "trhip_film_sum", "trhip_sample_map_default_params"):
        fns[name] = getattr(L, name)
        fns[name].restype, fns[name].argtypes = jr.ctypes_sig(calls[name][0])
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    err = lambda: T.lib().trhip_last_error(None)  # noqa: E731
    p = T._ffi.SampleMapParams()
    assert fns["trhip_sample_map_default_params"](C.addressof(p)) == 0 and p.pilot == 8
    mv, counts, total, film = np.ones((2, 3, 2), F), np.zeros(6, np.uint32), np.zeros(1, np.uint64), np.zeros((2, 3, 4), F)
    sn = T.scenes.shadows_camera(4).sensor()
    assert fns["trhip_render_path_map"](None, None, C.addressof(sn), vp(counts), 2, 4, 1, 0, vp(film), None) == -1 and b"null argument" in err()
    assert fns["trhip_last_sample_stats"](None, vp(mv)) == -1 and b"null argument" in err()
    assert fns["trhip_sample_map"](None, vp(mv), 3, 2, C.addressof(p), vp(counts), vp(total)) == -1 and b"null argument" in err()
    p.tau = -1.0  # the parameter block is read first: the bad field is named
    assert fns["trhip_sample_map"](None, vp(mv), 3, 2, C.addressof(p), vp(counts), vp(total)) == -1 and b"trhip_sample_map: tau" in err()
    assert fns["trhip_film_sum"](None, vp(film), vp(film), 3, 2, vp(film)) == -1 and b"null argument" in err()
    assert not counts.any() and not total.any() and not film.any()
