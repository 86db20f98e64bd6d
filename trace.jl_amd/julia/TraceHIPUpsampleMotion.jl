# TraceHIPUpsampleMotion.jl — temporal upsampling for a scene whose rigid bodies move; included by TraceHIP.jl inside `module TraceHIP`, after TraceHIPClipMotion.jl, and not
# loadable on its own.  It uses the module's LIB, check, context and TrhipStats, TemporalUpsampler and temporal_upsample_params of TraceHIPTemporalUpsample.jl and TrhipAovId
# of TraceHIPMotion.jl.  Its ccalls are checked against include/tracehip.h and written down in tests/golden/julia_shim_upsample_motion_calls.json
# (tests/test_julia_shim_upsample_motion.py).

# trhip_temporal_upsample_motion_params (128 bytes): trhip_temporal_upsample_params' fields (base), then the counts
mutable struct TrhipTemporalUpsampleMotionParams
    lo_from_hi::NTuple{4,Float32}
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    guide_sigma_normal::Float32
    guide_sigma_plane::Float32
    confidence_floor::Float32
    confidence_sharpness::Float32
    radius::UInt32
    flags::UInt32
    reserved::NTuple{2,UInt32}
    n_prims::UInt32
    n_bodies::UInt32
    motion_flags::UInt32
    reserved2::UInt32
end

# The library's defaults (trhip_temporal_upsample_motion_default_params; no context, no GPU), then what temporal_upsample_params sets for the same upsampler, map and camera
function temporal_upsample_motion_params(t::TemporalUpsampler, map::NTuple{4,Float32}, prev_camera, n_prims::Integer, n_bodies::Integer)
    p = TrhipTemporalUpsampleMotionParams(ntuple(_ -> 0f0, 4), ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0, 0, (UInt32(0), UInt32(0)), 0, 0, 0, 0)
    check(ccall((:trhip_temporal_upsample_motion_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    b = temporal_upsample_params(t, map, prev_camera)
    p.lo_from_hi, p.prev_world_to_pixel = b.lo_from_hi, b.prev_world_to_pixel
    p.radius, p.max_history, p.confidence_floor, p.confidence_sharpness = b.radius, b.max_history, b.confidence_floor, b.confidence_sharpness
    p.n_prims, p.n_bodies = n_prims, n_bodies
    p
end

# TemporalUpsampler's call for a scene whose rigid bodies moved (trhip_temporal_upsample_motion; docs/design/22-upsample-motion.md): a moving body keeps its full-size history.
# The images as in the upsampler's own call; ids: the FULL-SIZE frame's id plane (w x h records), `nothing` when body_of_prim is: every pixel is then static; body_of_prim and
# bodies as in accumulate_motion.  Returns (xyzw, history, mask).
function accumulate_upsample_motion(t::TemporalUpsampler, lo_xyzw::Array{Float32}, lo_planes::Array{Float32}, lo_width::Integer, lo_height::Integer, hi_planes::Array{Float32},
                                    history::Union{Nothing,Array{Float32}}, ids::Union{Nothing,Array{TrhipAovId}}, body_of_prim::Union{Nothing,Vector{UInt32}},
                                    bodies::Union{Nothing,Vector{NTuple{12,Float32}}}, width::Integer, height::Integer, map::NTuple{4,Float32}, prev_camera)
    length(lo_xyzw) == 4 * lo_width * lo_height && length(lo_planes) == 12 * lo_width * lo_height && length(hi_planes) == 12 * width * height ||
        error("TraceHIP: lo_xyzw must hold 4, lo_planes and hi_planes 12 floats per pixel")
    history === nothing || length(history) == length(hi_planes) || error("TraceHIP: history must have the size of hi_planes")
    ids === nothing || length(ids) == width * height || error("TraceHIP: ids must hold one record per full-size pixel")
    ids === nothing && body_of_prim !== nothing && error("TraceHIP: a body table needs the id plane")
    out, out_history, mask = Array{Float32}(undef, 4, width, height), similar(hi_planes), Array{UInt8}(undef, width, height)
    stats = TrhipStats()
    prm = temporal_upsample_motion_params(t, map, history === nothing ? nothing : prev_camera, body_of_prim === nothing ? 0 : length(body_of_prim),
                                          bodies === nothing ? 0 : length(bodies))
    rc = GC.@preserve prm history ids body_of_prim bodies ccall((:trhip_temporal_upsample_motion, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32},
         Ptr{Float32}, Ptr{UInt8}, Ptr{TrhipStats}),
        context(), lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history),
        ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids)), body_of_prim === nothing ? Ptr{UInt32}(C_NULL) : pointer(body_of_prim),
        bodies === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(bodies)), width, height, pointer_from_objref(prm), out, out_history, mask, Ref(stats))
    check(rc)
    out, out_history, mask
end
