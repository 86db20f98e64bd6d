"""trace.jl_amd/julia/TraceHIPTemporalUpsample.jl (the temporal-upsampling part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_display.py checks
TraceHIPDisplay.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the parameter struct mirrors the header's, the manifest
tests/golden/julia_shim_temporal_upsample_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPDisplay.jl, and jitter_for
holds the sequences of the Python TemporalUpsampler."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporalUpsample.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_temporal_upsample_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{4,Float32}": C.c_float * 4, "NTuple{12,Float32}": C.c_float * 12, "NTuple{2,UInt32}": C.c_uint32 * 2}


def test_every_temporal_upsample_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPTemporalUpsample.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_temporal_upsample", "trhip_temporal_upsample_default_params"]
    assert calls["trhip_temporal_upsample"][0][1][-4:] == ["ptr:f32", "ptr:f32", "ptr:u8", "ptr:stats"], "the film, the history, the mask (a byte image), the stats"


def test_julia_params_mirror_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalUpsampleParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S = T._ffi.TemporalUpsampleParams
    assert [n for n, _ in fields] == [n for n, _ in S._fields_]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in S._fields_]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(S, n).offset for n, _ in S._fields_] and offsets[-1] == C.sizeof(S) == 112


def test_temporal_upsample_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPTemporalUpsample.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPTemporalUpsample.jl changed: bring tests/golden/julia_shim_temporal_upsample_calls.json in step with its ccalls"


def test_the_shim_includes_the_temporal_upsample_file_after_the_display_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPTemporalUpsample.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPDisplay.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_julia_jitter_for_is_the_python_one(T):
    """The same sequences, term for term: the text of the Julia functions holds them."""
    src = open(SHIM, encoding="utf-8").read()
    body = src[src.index("function jitter_for("):]
    body = body[:body.index("\nend")]
    assert "((0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25))[frame % 4 + 1]" in body
    assert tuple(T.TemporalUpsampler.GRID) == ((0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25))
    assert "factor == 2 ||" in body and "t.jitter === nothing && return (0.0, 0.0)" in body
    assert "(radical_inverse(2, frame + 1) - 0.5, radical_inverse(3, frame + 1) - 0.5)" in body
    inverse = src[src.index("function radical_inverse("):]
    inverse = inverse[:inverse.index("\nend")]
    for line in ("f, r = 1.0, 0.0", "f /= base", "r += f * (i % base)", "i = div(i, base)"):
        assert line in inverse, line
