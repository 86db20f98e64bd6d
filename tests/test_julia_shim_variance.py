"""trace.jl_amd/julia/TraceHIPVariance.jl (the variance part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_temporal.py checks TraceHIPTemporal.jl,
without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the two parameter structs mirror the header's (their nested blocks written out field by field),
the manifest tests/golden/julia_shim_variance_calls.json is the one the source produces, TraceHIP.jl includes the file inside its module after the files it builds on."""
import ctypes as C
import json
import os
import re

import numpy as np

import julia_replay as jr

VARIANCE_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPVariance.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_variance_calls.json")
CT = {"Float32": C.c_float, "UInt32": C.c_uint32, "NTuple{12,Float32}": C.c_float * 12, "NTuple{2,UInt32}": C.c_uint32 * 2}


def test_every_variance_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(VARIANCE_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPVariance.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_denoise_var", "trhip_denoise_var_default_params", "trhip_temporal_moments", "trhip_temporal_moments_default_params"]


def julia_fields(name):
    src = open(VARIANCE_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct %s\n(.*?)\nend" % name, src, re.S).group(1)
    return re.findall(r"^\s+(\w+)::([\w{},]+)", body, re.M)


def flattened(S, Base):
    """(name, ctype, offset) of S's fields with its first field, a Base block, written out (flags and reserved as base_flags, base_reserved)."""
    flat = [("base_" + n if n in ("flags", "reserved") else n, c, S.base.offset + getattr(Base, n).offset) for n, c in Base._fields_]
    return flat + [(n, c, getattr(S, n).offset) for n, c in S._fields_[1:]]


def check_mirror(fields, flat, size):
    assert [n for n, _ in fields] == [n for n, _, _ in flat]
    assert [C.sizeof(CT[t]) for _, t in fields] == [C.sizeof(c) for _, c, _ in flat]
    offsets = np.cumsum([0] + [C.sizeof(CT[t]) for _, t in fields])  # every field is 4-byte aligned: Julia and C pack them alike
    assert list(offsets[:-1]) == [o for _, _, o in flat] and offsets[-1] == size


def test_julia_params_mirror_the_header(T):
    check_mirror(julia_fields("TrhipTemporalMomentsParams"), flattened(T._ffi.TemporalMomentsParams, T._ffi.TemporalParams), 88)
    check_mirror(julia_fields("TrhipDenoiseVarParams"), flattened(T._ffi.DenoiseVarParams, T._ffi.DenoiseParams), 48)
    assert C.sizeof(T._ffi.TemporalMomentsParams) == 88 and C.sizeof(T._ffi.DenoiseVarParams) == 48


def test_variance_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(VARIANCE_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPVariance.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPVariance.jl changed: bring tests/golden/julia_shim_variance_calls.json in step with its ccalls"


def test_the_shim_includes_the_variance_file_after_the_files_it_uses():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPVariance.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPTemporal.jl")') < src.index('include("TraceHIPTemporalClip.jl")') < at < src.rindex("end # module")
    temporal = open(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPTemporal.jl"), encoding="utf-8").read()
    for name in ("struct TemporalAccumulator", "function temporal_params("):  # what the variance file uses of the file before it
        assert name in temporal, name
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}
