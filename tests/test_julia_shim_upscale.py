"""trace.jl_amd/julia/TraceHIPUpscale.jl (the upscaling part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_variance.py checks
TraceHIPVariance.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the parameter struct mirrors the header's, the manifest
tests/golden/julia_shim_upscale_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPVariance.jl."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

UPSCALE_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPUpscale.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_upscale_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{4,Float32}": C.c_float * 4, "NTuple{2,UInt32}": C.c_uint32 * 2}


def test_every_upscale_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(UPSCALE_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPUpscale.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_upscale", "trhip_upscale_default_params"]
    assert calls["trhip_upscale"][0][1][-2:] == ["ptr:u8", "ptr:stats"], "the mask is a byte image"


def test_julia_params_mirror_the_header(T):
    src = open(UPSCALE_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipUpscaleParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S = T._ffi.UpscaleParams
    assert [n for n, _ in fields] == [n for n, _ in S._fields_]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in S._fields_]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(S, n).offset for n, _ in S._fields_] and offsets[-1] == C.sizeof(S) == 48


def test_upscale_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(UPSCALE_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPUpscale.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPUpscale.jl changed: bring tests/golden/julia_shim_upscale_calls.json in step with its ccalls"


def test_the_shim_includes_the_upscale_file_after_the_variance_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPUpscale.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPVariance.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_julia_pixel_map_is_the_python_one():
    """The same formula, term for term (Float64, one rounding per entry): the text of the Julia function holds it."""
    src = open(UPSCALE_SHIM, encoding="utf-8").read()
    body = src[src.index("function pixel_map("):]
    body = body[:body.index("\nend")]
    assert "Float64(lo.resolution[k]) / Float64(hi.resolution[k])" in body
    assert "-Float64(mh[t]) / Float64(mh[d]), -Float64(ml[t]) / Float64(ml[d])" in body
    assert "(Float64(hi.crop_bounds.p_min[k]) + 0.5 - o_hi) * a + o_lo - 0.5 - Float64(lo.crop_bounds.p_min[k])" in body
    assert "Float32(a), Float32(b)" in body
