"""trace.jl_amd/julia/TraceHIPMotion.jl (the moving-geometry part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_temporal_upsample.py checks
TraceHIPTemporalUpsample.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the parameter struct and the id record mirror the header's, the
manifest tests/golden/julia_shim_motion_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPTemporalUpsample.jl, and
prev_from_cur reads the rows the Python TemporalAccumulator.prev_from_cur reads."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPMotion.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_motion_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "Int32": C.c_int32, "NTuple{12,Float32}": C.c_float * 12}


def test_every_motion_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPMotion.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_render_aov_ids", "trhip_scene_free", "trhip_temporal_motion", "trhip_temporal_motion_default_params"]
    assert calls["trhip_temporal_motion"][0][1][4:7] == ["ptr:void", "ptr:u32", "ptr:f32"], "the id plane (records), the body table (words), the matrices (floats)"
    assert calls["trhip_render_aov_ids"][0][1][-4:] == ["ptr:f32", "ptr:void", "ptr:void", "ptr:stats"], "planes, records, the id plane, the stats"


def test_julia_structs_mirror_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalMotionParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    S = T._ffi.TemporalMotionParams
    assert [n for n, _ in fields] == [n for n, _ in S._fields_]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c in S._fields_]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [getattr(S, n).offset for n, _ in S._fields_] and offsets[-1] == C.sizeof(S) == 80
    body = re.search(r"\nstruct TrhipAovId\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    dt = T._ffi.AOV_ID_DTYPE
    assert [n for n, _ in fields] == list(dt.names) and [C.sizeof(CT[t]) for _, t in fields] == [dt.fields[n][0].itemsize for n in dt.names] == [4] * 4
    assert [t for _, t in fields] == ["Int32", "Int32", "Float32", "UInt32"]
    assert "const STATIC_BODY = 0xffffffff" in src and T._ffi.STATIC_BODY == 0xFFFFFFFF


def test_motion_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPMotion.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPMotion.jl changed: bring tests/golden/julia_shim_motion_calls.json in step with its ccalls"


def test_the_shim_includes_the_motion_file_after_the_temporal_upsample_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPMotion.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPTemporalUpsample.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_julia_prev_from_cur_is_the_python_one(T):
    """The same twelve numbers: rows 1-3 of the motion's inverse, row-major; the text of the Julia function holds the order."""
    src = open(SHIM, encoding="utf-8").read()
    assert "prev_from_cur(motion) = NTuple{12,Float32}(Float32(motion.inv_m[i, j]) for i in 1:3 for j in 1:4)" in src
    t = T.Transformation(np.arange(16, dtype=np.float32).reshape(4, 4) + np.eye(4, dtype=np.float32), np.arange(100, 116, dtype=np.float32).reshape(4, 4))
    assert T.TemporalAccumulator.prev_from_cur(t).reshape(-1).tolist() == [float(100 + 4 * i + j) for i in range(3) for j in range(4)]
    # the accumulator's fields that the Julia function copies are the four the Python one copies
    body = src[src.index("function temporal_motion_params("):]
    body = body[:body.index("\nend")]
    for name in ("max_history", "sigma_normal", "sigma_plane", "min_coverage"):
        assert f"t.{name} === nothing || (p.{name} = t.{name})" in body
    assert "p.n_prims, p.n_bodies = n_prims, n_bodies" in body
