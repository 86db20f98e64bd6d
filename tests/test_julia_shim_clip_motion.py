"""trace.jl_amd/julia/TraceHIPClipMotion.jl (the clip-with-motion part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_motion.py checks
TraceHIPMotion.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the parameter struct mirrors the header's 96 bytes, the manifest
tests/golden/julia_shim_clip_motion_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPMotion.jl, and the Julia
parameter function copies the fields the Python one copies."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPClipMotion.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_clip_motion_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{12,Float32}": C.c_float * 12}


def test_every_clip_motion_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPClipMotion.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_temporal_clip_motion", "trhip_temporal_clip_motion_default_params"]
    assert calls["trhip_temporal_clip_motion"][0][1][4:7] == ["ptr:void", "ptr:u32", "ptr:f32"], "the id plane (records), the body table (words), the matrices (floats)"
    motion = jr.parse_ccalls(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPMotion.jl"))
    assert calls["trhip_temporal_clip_motion"] == motion["trhip_temporal_motion"], "trhip_temporal_motion's arguments, in its order"


def test_julia_struct_mirrors_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalClipMotionParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S, B = T._ffi.TemporalClipMotionParams, T._ffi.TemporalMotionParams
    flat = list(B._fields_) + list(S._fields_[1:])  # base's fields in place, then the clip's
    assert [n for n, _ in fields] == [n for n, _ in flat]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in flat]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(B, n).offset for n, _ in B._fields_] + [getattr(S, n).offset for n, _ in S._fields_[1:]] and offsets[-1] == C.sizeof(S) == 96
    assert [t for n, t in fields if n in ("clip_gamma", "clip_radius", "clip_max_history", "reserved2")] == ["Float32", "UInt32", "Float32", "UInt32"]
    # the constructor call in the defaults function has one argument per field
    ctor = re.search(r"TrhipTemporalClipMotionParams\((ntuple\(_ -> 0f0, 12\)), ([^)]*)\)", src)
    assert ctor and len(ctor.group(2).split(",")) == len(fields) - 1


def test_clip_motion_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPClipMotion.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPClipMotion.jl changed: bring tests/golden/julia_shim_clip_motion_calls.json in step with its ccalls"


def test_the_shim_includes_the_clip_motion_file_after_the_motion_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPClipMotion.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPTemporalClip.jl")') < src.index('include("TraceHIPMotion.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_julia_parameter_function_copies_what_the_python_one_copies(T):
    src = open(SHIM, encoding="utf-8").read()
    body = src[src.index("function temporal_clip_motion_params("):]
    body = body[:body.index("\nend")]
    assert "p = temporal_clip_motion_default_params()" in body and "b = temporal_params(t.base, prev_camera)" in body
    assert "p.prev_world_to_pixel, p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage = b.prev_world_to_pixel, b.max_history, b.sigma_normal, b.sigma_plane, b.min_coverage" in body
    for name in ("clip_gamma", "clip_radius"):
        assert f"t.{name} === nothing || (p.{name} = t.{name})" in body
    assert "clip_max_history === nothing || (p.clip_max_history = clip_max_history)" in body and "p.n_prims, p.n_bodies = n_prims, n_bodies" in body
    # the Python accumulator fills the same block
    p = T.TemporalAccumulator(max_history=4, clip_gamma=0.5, clip_radius=1, carry_bodies=True, clip_max_history=2.0)._clip_motion_params_for(None, 7, 2)
    assert (p.base.max_history, p.base.n_prims, p.base.n_bodies, p.clip_gamma, p.clip_radius, p.clip_max_history, p.reserved2) == (4.0, 7, 2, 0.5, 1, 2.0, 0)
    # ids may be absent only with the table absent
    call = src[src.index("function accumulate_clip_motion("):]
    assert "ids === nothing && body_of_prim !== nothing && error(" in call and "ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids))" in call
