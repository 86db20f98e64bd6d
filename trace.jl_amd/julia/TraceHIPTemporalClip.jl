# TraceHIPTemporalClip.jl — temporal reprojection with variance clipping of the history; included by TraceHIP.jl inside `module TraceHIP`, after TraceHIPTemporal.jl, and not
# loadable on its own.  It uses that file's TrhipTemporalParams, TemporalAccumulator and temporal_params and the module's LIB, check, context and TrhipStats.  Its ccalls are
# checked against include/tracehip.h and written down in tests/golden/julia_shim_temporal_clip_calls.json (tests/test_temporal_clip_api.py).

# trhip_temporal_clip_params (88 bytes).  `base` is written out field by field — TrhipTemporalParams is mutable, so a field of that type would be a reference, not the 72 bytes —
# with its flags and reserved words as base_flags and base_reserved; then the new fields
mutable struct TrhipTemporalClipParams
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    base_flags::UInt32
    base_reserved::UInt32
    clip_gamma::Float32
    clip_radius::UInt32
    flags::UInt32
    reserved::UInt32
end

# A TemporalAccumulator whose reprojected history colour is first confined to mean +- clip_gamma * sd of the new frame's colours in a window of (2 clip_radius + 1)^2 pixels
# (trhip_temporal_clip; docs/design/15-temporal-clip.md).  `nothing` leaves a field at the library's default; clip_gamma = Inf32 gives `base`'s result bit for bit.
struct ClippedTemporalAccumulator
    base::TemporalAccumulator
    clip_gamma::Union{Nothing,Float32}
    clip_radius::Union{Nothing,UInt32}
    ClippedTemporalAccumulator(base::TemporalAccumulator = TemporalAccumulator(); clip_gamma = nothing, clip_radius = nothing) = new(base, clip_gamma, clip_radius)
end
function temporal_clip_params(t::ClippedTemporalAccumulator, prev_camera)
    p = TrhipTemporalClipParams(ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0, 0, 0f0, 0, 0, 0)
    check(ccall((:trhip_temporal_clip_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    b = temporal_params(t.base, prev_camera)  # the library's defaults for base are trhip_temporal_default_params'
    p.prev_world_to_pixel, p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage = b.prev_world_to_pixel, b.max_history, b.sigma_normal, b.sigma_plane, b.min_coverage
    t.clip_gamma === nothing || (p.clip_gamma = t.clip_gamma)
    t.clip_radius === nothing || (p.clip_radius = t.clip_radius)
    p
end

# As TemporalAccumulator's call: xyzw 4 x w x h Float32, planes and history 4 x 3 x w x h; returns (xyzw, history) of this frame.  After a change of lights the history may be
# kept: it is cut back to the new frame's colours within a frame.
function (t::ClippedTemporalAccumulator)(xyzw::Array{Float32}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}}, prev_camera, width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height || error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel")
    history === nothing || length(history) == length(planes) || error("TraceHIP: history must have the size of planes")
    out, out_history = similar(xyzw), similar(planes)
    stats = TrhipStats()
    prm = temporal_clip_params(t, history === nothing ? nothing : prev_camera)
    rc = GC.@preserve prm history ccall((:trhip_temporal_clip, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), width, height, pointer_from_objref(prm), out, out_history, Ref(stats))
    check(rc)
    out, out_history
end
