# TraceHIPClipMotion.jl — clipped temporal reprojection for a scene whose rigid bodies move; included by TraceHIP.jl inside `module TraceHIP`, after TraceHIPMotion.jl, and not
# loadable on its own.  It uses the module's LIB, check, context and TrhipStats, TemporalAccumulator and temporal_params of TraceHIPTemporal.jl,
# ClippedTemporalAccumulator of TraceHIPTemporalClip.jl and TrhipAovId of TraceHIPMotion.jl.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_clip_motion_calls.json (tests/test_julia_shim_clip_motion.py).

# trhip_temporal_clip_motion_params (96 bytes): trhip_temporal_motion_params' fields (base), then the clip's
mutable struct TrhipTemporalClipMotionParams
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    n_prims::UInt32
    n_bodies::UInt32
    flags::UInt32
    reserved::UInt32
    clip_gamma::Float32
    clip_radius::UInt32
    clip_max_history::Float32
    reserved2::UInt32
end

# The library's defaults (trhip_temporal_clip_motion_default_params; no context, no GPU)
function temporal_clip_motion_default_params()
    p = TrhipTemporalClipMotionParams(ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0, 0, 0, 0, 0f0, 0, 0f0, 0)
    check(ccall((:trhip_temporal_clip_motion_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p
end

# `clip_max_history`: a pixel whose history colour was clipped has its history length cut to this before the blend; `nothing` leaves the library's default, Inf32 never cuts
function temporal_clip_motion_params(t::ClippedTemporalAccumulator, clip_max_history, prev_camera, n_prims::Integer, n_bodies::Integer)
    p = temporal_clip_motion_default_params()
    b = temporal_params(t.base, prev_camera)  # the library's defaults for base are trhip_temporal_default_params'
    p.prev_world_to_pixel, p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage = b.prev_world_to_pixel, b.max_history, b.sigma_normal, b.sigma_plane, b.min_coverage
    t.clip_gamma === nothing || (p.clip_gamma = t.clip_gamma)
    t.clip_radius === nothing || (p.clip_radius = t.clip_radius)
    clip_max_history === nothing || (p.clip_max_history = clip_max_history)
    p.n_prims, p.n_bodies = n_prims, n_bodies
    p
end

# ClippedTemporalAccumulator's call for a scene whose rigid bodies moved (trhip_temporal_clip_motion; docs/design/21-clip-motion.md): a moving body keeps its history and the
# shadow it drags over static surfaces is cut back to the new frame's colours.  Arguments as accumulate_motion's; ids may be `nothing` when body_of_prim is: every pixel is
# then static.  Returns (xyzw, history).
function accumulate_clip_motion(t::ClippedTemporalAccumulator, xyzw::Array{Float32}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}},
                                ids::Union{Nothing,Array{TrhipAovId}}, body_of_prim::Union{Nothing,Vector{UInt32}}, bodies::Union{Nothing,Vector{NTuple{12,Float32}}}, prev_camera,
                                width::Integer, height::Integer; clip_max_history = nothing)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height || error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel")
    ids === nothing || length(ids) == width * height || error("TraceHIP: ids must hold one record per pixel")
    ids === nothing && body_of_prim !== nothing && error("TraceHIP: a body table needs the id plane")
    history === nothing || length(history) == length(planes) || error("TraceHIP: history must have the size of planes")
    out, out_history = similar(xyzw), similar(planes)
    stats = TrhipStats()
    prm = temporal_clip_motion_params(t, clip_max_history, history === nothing ? nothing : prev_camera, body_of_prim === nothing ? 0 : length(body_of_prim),
                                      bodies === nothing ? 0 : length(bodies))
    rc = GC.@preserve prm history ids body_of_prim bodies ccall((:trhip_temporal_clip_motion, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), ids === nothing ? C_NULL : Ptr{Cvoid}(pointer(ids)),
        body_of_prim === nothing ? Ptr{UInt32}(C_NULL) : pointer(body_of_prim), bodies === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(bodies)), width, height,
        pointer_from_objref(prm), out, out_history, Ref(stats))
    check(rc)
    out, out_history
end
