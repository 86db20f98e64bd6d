"""trace.jl_amd/julia/TraceHIPTemporal.jl (the temporal-reprojection part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_ao.py checks
TraceHIPAO.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, TrhipTemporalParams mirrors trhip_temporal_params, the manifest
tests/golden/julia_shim_temporal_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module, and its own manifest is untouched."""
import ctypes as C
import json
import os
import re

import julia_replay as jr

TEMPORAL_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporal.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_temporal_calls.json")


def test_every_temporal_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(TEMPORAL_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPTemporal.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_sensor_world_to_pixel", "trhip_temporal", "trhip_temporal_default_params"]


def test_temporal_params_mirror_the_header():
    import __graft_entry__ as graft
    T = graft.load_package()
    src = open(TEMPORAL_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipTemporalParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)
    ct = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{12,Float32}": C.c_float * 12}
    mirror = list(T._ffi.TemporalParams._fields_)
    assert [n for n, _ in fields] == [n for n, _ in mirror]
    assert [C.sizeof(ct[t]) for _, t in fields] == [C.sizeof(c) for _, c in mirror]
    assert sum(C.sizeof(ct[t]) for _, t in fields) == C.sizeof(T._ffi.TemporalParams) == 72


def test_temporal_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(TEMPORAL_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPTemporal.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPTemporal.jl changed: bring tests/golden/julia_shim_temporal_calls.json in step with its ccalls"


def test_the_shim_includes_the_temporal_file_inside_its_module():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPTemporal.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPAO.jl")') < at < src.rindex("end # module")
    # the names the included file uses are defined before it
    for name in ("mutable struct TrhipStats", "struct TrhipSensor", "function context()", "check(rc) =", "function sensor("):
        assert 0 <= src.index(name) < at, name
