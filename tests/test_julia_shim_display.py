"""trace.jl_amd/julia/TraceHIPDisplay.jl (the display part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_upscale.py checks
TraceHIPUpscale.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the two structs mirror the header's, the manifest
tests/golden/julia_shim_display_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPUpscale.jl."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import julia_replay as jr

DISPLAY_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPDisplay.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_display_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{2,UInt32}": C.c_uint32 * 2}


def test_every_display_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(DISPLAY_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPDisplay.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_display", "trhip_display_default_params", "trhip_display_srgb_table"]
    assert calls["trhip_display"][0][1][-3:] == ["ptr:u8", "ptr:u32", "ptr:stats"], "the bytes, the histogram, the stats"
    assert calls["trhip_display"][0][1][4] == "f32", "scale travels as a Float32"


@pytest.mark.parametrize("julia_name, ffi_name, size", [("TrhipDisplayParams", "DisplayParams", 48), ("TrhipDisplayState", "DisplayState", 16)])
def test_julia_structs_mirror_the_header(T, julia_name, ffi_name, size):
    src = open(DISPLAY_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct " + julia_name + r"\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S = getattr(T._ffi, ffi_name)
    assert [n for n, _ in fields] == [n for n, _ in S._fields_]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in S._fields_]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(S, n).offset for n, _ in S._fields_] and offsets[-1] == C.sizeof(S) == size


def test_display_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(DISPLAY_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPDisplay.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPDisplay.jl changed: bring tests/golden/julia_shim_display_calls.json in step with its ccalls"


def test_the_shim_includes_the_display_file_after_the_upscale_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPDisplay.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPUpscale.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}
