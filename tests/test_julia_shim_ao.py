"""trace.jl_amd/julia/TraceHIPAO.jl (the ambient-occlusion part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim.py checks
TraceHIP.jl itself, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, TrhipAoParams mirrors trhip_ao_params, the manifest
tests/golden/julia_shim_ao_calls.json is the one the source produces, and TraceHIP.jl includes the file inside its module."""
import ctypes as C
import json
import os
import re

import julia_replay as jr

AO_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPAO.jl")
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "julia_shim_ao_calls.json")


def test_every_ao_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(AO_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPAO.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_ao_default_params", "trhip_render_ao", "trhip_render_ao_device", "trhip_film_reduce", "trhip_scene_free"):
        assert need in calls, need


def test_ao_params_mirror_the_header():
    import __graft_entry__ as graft
    T = graft.load_package()
    src = open(AO_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipAoParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    ct = {"Float32": C.c_float, "UInt32": C.c_uint32}
    assert [(n, ct[t]) for n, t in fields] == list(T._ffi.AoParams._fields_)
    assert sum(C.sizeof(ct[t]) for _, t in fields) == C.sizeof(T._ffi.AoParams) == 16
    assert int(re.search(r"const TRHIP_AO_ALBEDO = UInt32\((\d+)\)", src).group(1)) == T._ffi.AO_ALBEDO


def test_ao_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(AO_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPAO.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPAO.jl changed: bring tests/golden/julia_shim_ao_calls.json in step with its ccalls"


def test_the_shim_includes_the_ao_file_inside_its_module():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPAO.jl")')
    assert src.index("module TraceHIP") < at < src.rindex("end # module")
    # the names the included file uses are defined before it
    for name in ("mutable struct TrhipStats", "function context()", "check(rc) =", "function flatten(", "function sensor(", "seed_of(", "const JOB", "function shard_samples(",
                 "function write_film!("):
        assert 0 <= src.index(name) < at, name
