# TraceHIPTemporal.jl — temporal reprojection for moving-camera previews; included by TraceHIP.jl inside `module TraceHIP`, after TraceHIPAO.jl, and not loadable on its own.
# It uses the module's LIB, check, context, sensor, TrhipSensor and TrhipStats.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_temporal_calls.json (tests/test_julia_shim_temporal.py), as TraceHIP.jl's own are in julia_shim_calls.json.

# trhip_temporal_params (72 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipTemporalParams
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    flags::UInt32
    reserved::UInt32
end

# The previous camera's matrix (include/tracehip.h, trhip_sensor_world_to_pixel): row-major 3 x 4, h = M (p, 1), (h.x / h.z, h.y / h.z) the position of the world point p in
# film-array pixel coordinates — 0-based, integers at pixel centres; add 1 for Julia's film.pixels[y, x] —, valid iff h.z > 0.  Host arithmetic: no context, no GPU.
function world_to_pixel(camera::Trace.PerspectiveCamera)
    sn = Ref(sensor(camera))
    out = Vector{Float32}(undef, 12)
    check(ccall((:trhip_sensor_world_to_pixel, LIB), Cint, (Ptr{TrhipSensor}, Ptr{Float32}), sn, out))
    NTuple{12,Float32}(out)
end

# Blends a path film with the previous frame's accumulated colour, fetched through the previous camera and validated against the feature planes (trhip_temporal;
# docs/design/14-temporal.md).  `nothing` leaves a field at the library's default.
struct TemporalAccumulator
    max_history::Union{Nothing,Float32}
    sigma_normal::Union{Nothing,Float32}
    sigma_plane::Union{Nothing,Float32}
    min_coverage::Union{Nothing,Float32}
    TemporalAccumulator(; max_history = nothing, sigma_normal = nothing, sigma_plane = nothing, min_coverage = nothing) = new(max_history, sigma_normal, sigma_plane, min_coverage)
end
function temporal_params(t::TemporalAccumulator, prev_camera)
    p = TrhipTemporalParams(ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0, 0)
    check(ccall((:trhip_temporal_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    t.max_history === nothing || (p.max_history = t.max_history)
    t.sigma_normal === nothing || (p.sigma_normal = t.sigma_normal)
    t.sigma_plane === nothing || (p.sigma_plane = t.sigma_plane)
    t.min_coverage === nothing || (p.min_coverage = t.min_coverage)
    prev_camera === nothing || (p.prev_world_to_pixel = world_to_pixel(prev_camera))
    p
end

# xyzw: 4 x w x h Float32 (the film accumulators as the render calls write them), planes and history: 4 x 3 x w x h; history and prev_camera may be `nothing` (first frame, or
# after a change of lights: the pass does not detect one).  Returns (xyzw, history) of this frame; the xyzw goes into the denoiser with the same planes.
function (t::TemporalAccumulator)(xyzw::Array{Float32}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}}, prev_camera, width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height || error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel")
    history === nothing || length(history) == length(planes) || error("TraceHIP: history must have the size of planes")
    out, out_history = similar(xyzw), similar(planes)
    stats = TrhipStats()
    prm = temporal_params(t, history === nothing ? nothing : prev_camera)
    rc = GC.@preserve prm history ccall((:trhip_temporal, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), width, height, pointer_from_objref(prm), out, out_history, Ref(stats))
    check(rc)
    out, out_history
end
