"""trace.jl_amd/julia/TraceHIPDirectSplit.jl (the direct-split part of the shim, included by TraceHIP.jl) checked the way tests/test_julia_shim_upsample_motion.py checks
TraceHIPUpsampleMotion.jl, without a Julia runtime: every ccall binds a prototype of include/tracehip.h, the manifest tests/golden/julia_shim_direct_split_calls.json is the
one the source produces, TraceHIP.jl includes the file inside its module after TraceHIPUpsampleMotion.jl, the pass borrows TraceHIPMotion.jl's parameter function, and the
shim's own signatures, replayed through ctypes, reach the library's argument checks."""
import ctypes as C
import json
import os

import numpy as np

import julia_replay as jr

SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPDirectSplit.jl")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "julia_shim_direct_split_calls.json")
F = np.float32


def test_every_direct_split_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPDirectSplit.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    assert sorted(calls) == ["trhip_film_add", "trhip_temporal_split"]
    args = calls["trhip_temporal_split"][0][1]
    parent = jr.parse_ccalls(os.path.join(os.path.dirname(jr.SHIM), "TraceHIPMotion.jl"))["trhip_temporal_motion"][0][1]
    assert args[2] == "ptr:f32" and args[:2] + args[3:] == parent, "trhip_temporal_motion's arguments in its order, with the direct film directly after xyzw"
    assert calls["trhip_film_add"][0][1] == ["ptr:void", "ptr:f32", "ptr:f32", "u32", "u32", "ptr:f32", "ptr:stats"]


def test_direct_split_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPDirectSplit.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPDirectSplit.jl changed: bring tests/golden/julia_shim_direct_split_calls.json in step with its ccalls"


def test_the_shim_includes_the_direct_split_file_after_the_upsample_motion_file():
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPDirectSplit.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPMotion.jl")') < src.index('include("TraceHIPUpsampleMotion.jl")') < at < src.rindex("end # module")
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(GOLDEN, "julia_shim_calls.json")))
    calls = jr.parse_ccalls(jr.SHIM)
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}


def test_the_julia_call_fills_what_the_python_one_fills(T):
    src = open(SHIM, encoding="utf-8").read()
    call = src[src.index("function accumulate_split("):]
    call = call[:call.index("\nend")]
    # no parameter block of its own: TraceHIPMotion.jl's function, with the camera only when there is a history and the counts from the arrays
    assert "mutable struct" not in src
    assert ("prm = temporal_motion_params(t, history === nothing ? nothing : prev_camera, body_of_prim === nothing ? 0 : length(body_of_prim), "
            "bodies === nothing ? 0 : length(bodies))") in call
    p = T.TemporalAccumulator(max_history=4)._split_params_for(None, 7, 2)
    assert (p.max_history, p.n_prims, p.n_bodies, p.flags, p.reserved) == (4.0, 7, 2, 0, 0)
    # direct and ids may be absent; ids only with the table absent
    assert "direct === nothing ? Ptr{Float32}(C_NULL) : pointer(direct)" in call and "direct === nothing || length(direct) == length(xyzw) || error(" in call
    assert "ids === nothing && body_of_prim !== nothing && error(" in call and "ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids))" in call
    assert "GC.@preserve prm direct history ids body_of_prim bodies" in call


def test_the_shims_signatures_replayed_through_ctypes_reach_the_argument_checks(T):
    """The ccalls' own argument types, bound to the library through ctypes as Julia binds them, with a NULL context: the parameter block is read first (a bad field is named),
    then the null context is refused; nothing is written."""
    calls = jr.parse_ccalls(SHIM)
    L = C.CDLL(T.lib()._name)
    split, add = L.trhip_temporal_split, L.trhip_film_add
    split.restype, split.argtypes = jr.ctypes_sig(calls["trhip_temporal_split"][0])
    add.restype, add.argtypes = jr.ctypes_sig(calls["trhip_film_add"][0])
    w, h = 3, 2
    xyzw, direct, planes, out, out_h = np.ones((h, w, 4), F), np.ones((h, w, 4), F), np.ones((h, w, 3, 4), F), np.zeros((h, w, 4), F), np.zeros((h, w, 3, 4), F)
    p = T.TemporalAccumulator()._split_params_for(None, 0, 0)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert split(None, vp(xyzw), vp(direct), vp(planes), None, None, None, None, w, h, C.addressof(p), vp(out), vp(out_h), None) == -1
    assert b"null argument" in T.lib().trhip_last_error(None)
    p.sigma_plane = 0.0
    assert split(None, vp(xyzw), vp(direct), vp(planes), None, None, None, None, w, h, C.addressof(p), vp(out), vp(out_h), None) == -1
    assert b"trhip_temporal_split: sigma_plane" in T.lib().trhip_last_error(None)
    assert add(None, vp(xyzw), vp(direct), w, h, vp(out), None) == -1 and b"null argument" in T.lib().trhip_last_error(None)
    assert not out.any() and not out_h.any()
