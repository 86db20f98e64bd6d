# TraceHIPDirectSplit.jl — a preview that keeps the first-hit direct light out of its history; included by TraceHIP.jl inside `module TraceHIP`, after
# TraceHIPUpsampleMotion.jl, and not loadable on its own.  It uses the module's LIB, check, context and TrhipStats, TemporalAccumulator of TraceHIPTemporal.jl and TrhipAovId,
# temporal_motion_params of TraceHIPMotion.jl: the pass has no parameter block of its own.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_direct_split_calls.json (tests/test_julia_shim_direct_split.py).

# accumulate_motion on xyzw.xyz - direct.xyz (trhip_temporal_split; docs/design/23-direct-split.md).  direct: the film of the frame's first-hit direct light — the path frame at
# max_depth = 1 with the frame's sampler — or `nothing`: accumulate_motion's result bit for bit.  ids: this frame's aov_ids, `nothing` when body_of_prim is: every pixel is then
# static.  Returns (xyzw, history) of the indirect remainder; film_add puts the direct film back after the filter.
function accumulate_split(t::TemporalAccumulator, xyzw::Array{Float32}, direct::Union{Nothing,Array{Float32}}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}},
                          ids::Union{Nothing,Array{TrhipAovId}}, body_of_prim::Union{Nothing,Vector{UInt32}}, bodies::Union{Nothing,Vector{NTuple{12,Float32}}}, prev_camera,
                          width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height || error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel")
    direct === nothing || length(direct) == length(xyzw) || error("TraceHIP: direct must have the size of xyzw")
    history === nothing || length(history) == length(planes) || error("TraceHIP: history must have the size of planes")
    ids === nothing || length(ids) == width * height || error("TraceHIP: ids must hold one record per pixel")
    ids === nothing && body_of_prim !== nothing && error("TraceHIP: a body table needs the id plane")
    out, out_history = similar(xyzw), similar(planes)
    stats = TrhipStats()
    prm = temporal_motion_params(t, history === nothing ? nothing : prev_camera, body_of_prim === nothing ? 0 : length(body_of_prim), bodies === nothing ? 0 : length(bodies))
    rc = GC.@preserve prm direct history ids body_of_prim bodies ccall((:trhip_temporal_split, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32},
         Ptr{TrhipStats}),
        context(), xyzw, direct === nothing ? Ptr{Float32}(C_NULL) : pointer(direct), planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history),
        ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids)), body_of_prim === nothing ? Ptr{UInt32}(C_NULL) : pointer(body_of_prim),
        bodies === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(bodies)), width, height, pointer_from_objref(prm), out, out_history, Ref(stats))
    check(rc)
    out, out_history
end

# a.xyz + b.xyz with a's weight lane (trhip_film_add): the direct film back onto the filtered remainder
function film_add(a::Array{Float32}, b::Array{Float32}, width::Integer, height::Integer)
    length(a) == 4 * width * height && length(b) == length(a) || error("TraceHIP: both films must hold 4 floats per pixel")
    out = similar(a)
    stats = TrhipStats()
    check(ccall((:trhip_film_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Float32}, Ptr{TrhipStats}), context(), a, b, width, height, out, Ref(stats)))
    out
end
