"""trace.jl_amd/julia/TraceHIPUpsampleMotion.jl (the upsampling-with-motion part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_clip_motion.py
checks TraceHIPClipMotion.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the parameter struct mirrors the header's 128 bytes, the manifest
tests/golden/julia_shim_upsample_motion_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPClipMotion.jl, and the Julia
parameter function fills the block the Python one fills."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPUpsampleMotion.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_upsample_motion_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{12,Float32}": C.c_float * 12, "NTuple{4,Float32}": C.c_float * 4, "NTuple{2,UInt32}": C.c_uint32 * 2}


def test_every_upsample_motion_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPUpsampleMotion.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_temporal_upsample_motion", "trhip_temporal_upsample_motion_default_params"]
    args = calls["trhip_temporal_upsample_motion"][0][1]
    assert args[7:10] == ["ptr:void", "ptr:u32", "ptr:f32"], "the id plane (records), the body table (words), the matrices (floats), directly after history"
    parent = jr.parse_ccalls(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporalUpsample.jl"))["trhip_temporal_upsample"][0][1]
    assert args[:7] + args[10:] == parent, "trhip_temporal_upsample's arguments, in its order"


def test_julia_struct_mirrors_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalUpsampleMotionParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S, B = T._ffi.TemporalUpsampleMotionParams, T._ffi.TemporalUpsampleParams
    flat = list(B._fields_) + list(S._fields_[1:])  # base's fields in place, then the counts
    assert [n for n, _ in fields] == [n for n, _ in flat]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in flat]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(B, n).offset for n, _ in B._fields_] + [getattr(S, n).offset for n, _ in S._fields_[1:]] and offsets[-1] == C.sizeof(S) == 128
    assert [(n, int(o)) for (n, _), o in zip(fields, offsets)][-4:] == [("n_prims", 112), ("n_bodies", 116), ("motion_flags", 120), ("reserved2", 124)], "the header's offsets"
    # the base is the parent file's struct, field for field
    parent = open(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporalUpsample.jl"), encoding="utf-8").read()
    parent_fields = re.findall(r"^\s+(\w+)::([\w{},]+)", re.search(r"mutable struct TrhipTemporalUpsampleParams\n(.*?)\nend", parent, re.S).group(1), re.M)
    assert fields[:len(parent_fields)] == parent_fields
    # the constructor call in the parameter function has one argument per field
    ctor = re.search(r"TrhipTemporalUpsampleMotionParams\(ntuple\(_ -> 0f0, 4\), ntuple\(_ -> 0f0, 12\), (.*?), \(UInt32\(0\), UInt32\(0\)\), ([^)]*)\)", src)
    assert ctor and len(ctor.group(1).split(",")) + len(ctor.group(2).split(",")) == len(fields) - 3


def test_upsample_motion_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPUpsampleMotion.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPUpsampleMotion.jl changed: bring tests/golden/julia_shim_upsample_motion_calls.json in step with its ccalls"


def test_the_shim_includes_the_upsample_motion_file_after_the_clip_motion_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPUpsampleMotion.jl")')
    assert (src.index("module TraceHIP") < src.index('include("TraceHIPTemporalUpsample.jl")') < src.index('include("TraceHIPMotion.jl")')
            < src.index('include("TraceHIPClipMotion.jl")') < at < src.rindex("end # module"))
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_julia_parameter_function_fills_what_the_python_one_fills(T):
    src = open(SHIM, encoding="utf-8").read()
    body = src[src.index("function temporal_upsample_motion_params("):]
    body = body[:body.index("\nend")]
    assert ":trhip_temporal_upsample_motion_default_params" in body and "b = temporal_upsample_params(t, map, prev_camera)" in body
    assert "p.lo_from_hi, p.prev_world_to_pixel = b.lo_from_hi, b.prev_world_to_pixel" in body
    assert "p.radius, p.max_history, p.confidence_floor, p.confidence_sharpness = b.radius, b.max_history, b.confidence_floor, b.confidence_sharpness" in body
    assert "p.n_prims, p.n_bodies = n_prims, n_bodies" in body
    # the Python upsampler fills the same block
    p = T.TemporalUpsampler(radius=2, max_history=4, confidence_floor=0.5, confidence_sharpness=1.0, carry_bodies=True)._motion_params_for((0.5, 0.25, 0.5, -0.25), None, 7, 2)
    assert (p.base.radius, p.base.max_history, p.base.confidence_floor, p.base.confidence_sharpness, p.n_prims, p.n_bodies, p.motion_flags, p.reserved2) == (2, 4.0, 0.5, 1.0, 7, 2, 0, 0)
    # ids may be absent only with the table absent, and is the full-size frame's
    call = src[src.index("function accumulate_upsample_motion("):]
    assert "ids === nothing && body_of_prim !== nothing && error(" in call and "ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids))" in call
    assert "ids === nothing || length(ids) == width * height || error(" in call
