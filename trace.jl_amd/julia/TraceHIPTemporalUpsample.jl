# TraceHIPTemporalUpsample.jl — temporal upsampling of jittered low-resolution path frames into a full-size history; included by TraceHIP.jl inside `module TraceHIP`, after
# TraceHIPDisplay.jl, and not loadable on its own.  It uses the module's LIB, check, context and TrhipStats, world_to_pixel of TraceHIPTemporal.jl and pixel_map of
# TraceHIPUpscale.jl.  Its ccalls are checked against include/tracehip.h and written down in tests/golden/julia_shim_temporal_upsample_calls.json
# (tests/test_julia_shim_temporal_upsample.py).

# trhip_temporal_upsample_params (112 bytes)
mutable struct TrhipTemporalUpsampleParams
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
end

# `nothing` leaves a field at trhip_temporal_upsample_default_params'.  jitter: :grid (factor 2 only), :halton or nothing.
struct TemporalUpsampler
    radius::Union{Nothing,UInt32}
    max_history::Union{Nothing,Float32}
    confidence_floor::Union{Nothing,Float32}
    confidence_sharpness::Union{Nothing,Float32}
    jitter::Union{Nothing,Symbol}
    TemporalUpsampler(; radius = nothing, max_history = nothing, confidence_floor = nothing, confidence_sharpness = nothing, jitter = :grid) =
        new(radius, max_history, confidence_floor, confidence_sharpness, jitter)
end

# (jx, jy) of frame `frame` (0-based), in LOW-pixel units: the low camera of that frame is the camera with both corners of its screen window moved by (-jx, -jy), and its
# pixel_map is the unjittered one with bx + jx, by + jy (docs/design/19-temporal-upsample.md).  :grid — frame mod 4 gives (+1/4, +1/4), (-1/4, -1/4), (-1/4, +1/4),
# (+1/4, -1/4): with the 2 x map's fractional parts of 1/4 and 3/4 every full-size pixel centre lies on a low pixel centre once in four frames.  :halton — the radical
# inverses of frame + 1 in bases 2 and 3, minus 1/2.
function radical_inverse(base::Integer, i::Integer)
    f, r = 1.0, 0.0
    while i > 0
        f /= base
        r += f * (i % base)
        i = div(i, base)
    end
    r
end
function jitter_for(t::TemporalUpsampler, frame::Integer, factor = 2)
    frame >= 0 || error("TraceHIP: frame must be >= 0")
    t.jitter === nothing && return (0.0, 0.0)
    if t.jitter === :grid
        factor == 2 || error("TraceHIP: jitter :grid needs factor 2 (use :halton)")
        return ((0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25))[frame % 4 + 1]
    end
    t.jitter === :halton || error("TraceHIP: jitter must be :grid, :halton or nothing")
    (radical_inverse(2, frame + 1) - 0.5, radical_inverse(3, frame + 1) - 0.5)
end

function temporal_upsample_params(t::TemporalUpsampler, map::NTuple{4,Float32}, prev_camera)
    p = TrhipTemporalUpsampleParams(ntuple(_ -> 0f0, 4), ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0, 0, (UInt32(0), UInt32(0)))
    check(ccall((:trhip_temporal_upsample_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.lo_from_hi = map
    t.radius === nothing || (p.radius = t.radius)
    t.max_history === nothing || (p.max_history = t.max_history)
    t.confidence_floor === nothing || (p.confidence_floor = t.confidence_floor)
    t.confidence_sharpness === nothing || (p.confidence_sharpness = t.confidence_sharpness)
    prev_camera === nothing || (p.prev_world_to_pixel = world_to_pixel(prev_camera))  # the previous FULL-SIZE camera
    p
end

# lo_xyzw 4 x lw x lh Float32 and lo_planes 4 x 3 x lw x lh of this frame's jittered low camera, hi_planes and history 4 x 3 x w x h; history and prev_camera may be `nothing`.
# Returns (xyzw 4 x w x h, history, mask w x h: the upscaler's class + 4 where history was found).
function (t::TemporalUpsampler)(lo_xyzw::Array{Float32}, lo_planes::Array{Float32}, lo_width::Integer, lo_height::Integer, hi_planes::Array{Float32},
                                history::Union{Nothing,Array{Float32}}, width::Integer, height::Integer, map::NTuple{4,Float32}, prev_camera)
    length(lo_xyzw) == 4 * lo_width * lo_height && length(lo_planes) == 12 * lo_width * lo_height && length(hi_planes) == 12 * width * height ||
        error("TraceHIP: lo_xyzw must hold 4, lo_planes and hi_planes 12 floats per pixel")
    history === nothing || length(history) == length(hi_planes) || error("TraceHIP: history must have the size of hi_planes")
    out, out_history, mask = Array{Float32}(undef, 4, width, height), similar(hi_planes), Array{UInt8}(undef, width, height)
    stats = TrhipStats()
    prm = temporal_upsample_params(t, map, history === nothing ? nothing : prev_camera)
    rc = GC.@preserve prm history ccall((:trhip_temporal_upsample, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{TrhipStats}),
        context(), lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), width, height, pointer_from_objref(prm), out,
        out_history, mask, Ref(stats))
    check(rc)
    out, out_history, mask
end
