# TraceHIPVariance.jl — luminance moments along the reprojection and the variance-guided à-trous filter; included by TraceHIP.jl inside `module TraceHIP`, after
# TraceHIPTemporalClip.jl, and not loadable on its own.  It uses TraceHIPTemporal.jl's TemporalAccumulator and temporal_params and the module's LIB, check, context and
# TrhipStats.  Its ccalls are checked against include/tracehip.h and written down in tests/golden/julia_shim_variance_calls.json (tests/test_julia_shim_variance.py).

# trhip_temporal_moments_params (88 bytes).  `base` is written out field by field, as in TrhipTemporalClipParams; then the new fields
mutable struct TrhipTemporalMomentsParams
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    base_flags::UInt32
    base_reserved::UInt32
    albedo_floor::Float32
    spatial_below::Float32
    flags::UInt32
    reserved::UInt32
end

# trhip_denoise_var_params (48 bytes): trhip_denoise_params field by field (its flags and reserved as base_flags, base_reserved), then the new fields
mutable struct TrhipDenoiseVarParams
    iterations::UInt32
    base_flags::UInt32
    sigma_colour::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    albedo_floor::Float32
    min_coverage::Float32
    base_reserved::UInt32
    var_eps::Float32
    flags::UInt32
    reserved::NTuple{2,UInt32}
end

# A TemporalAccumulator that carries the two luminance moments along and returns a variance plane (trhip_temporal_moments; docs/design/16-variance.md).  `nothing` leaves a
# field at the library's default; `demodulate` must be the denoiser's.  The colour and the history it returns are `base`'s bit for bit.
struct MomentsTemporalAccumulator
    base::TemporalAccumulator
    spatial_below::Union{Nothing,Float32}
    albedo_floor::Union{Nothing,Float32}
    demodulate::Bool
    MomentsTemporalAccumulator(base::TemporalAccumulator = TemporalAccumulator(); spatial_below = nothing, albedo_floor = nothing, demodulate = true) =
        new(base, spatial_below, albedo_floor, demodulate)
end
function temporal_moments_params(t::MomentsTemporalAccumulator, prev_camera)
    p = TrhipTemporalMomentsParams(ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0, 0, 0f0, 0f0, 0, 0)
    check(ccall((:trhip_temporal_moments_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    b = temporal_params(t.base, prev_camera)  # the library's defaults for base are trhip_temporal_default_params'
    p.prev_world_to_pixel, p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage = b.prev_world_to_pixel, b.max_history, b.sigma_normal, b.sigma_plane, b.min_coverage
    t.spatial_below === nothing || (p.spatial_below = t.spatial_below)
    t.albedo_floor === nothing || (p.albedo_floor = t.albedo_floor)
    p.flags = t.demodulate ? UInt32(1) : UInt32(0)  # TRHIP_DENOISE_DEMODULATE
    p
end

# xyzw 4 x w x h Float32, planes and history 4 x 3 x w x h, moments 2 x w x h; history and moments are `nothing` together.  Returns (xyzw, history, moments, variance w x h).
function (t::MomentsTemporalAccumulator)(xyzw::Array{Float32}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}}, moments::Union{Nothing,Array{Float32}}, prev_camera,
                                         width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height || error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel")
    (history === nothing) == (moments === nothing) || error("TraceHIP: moments must be nothing exactly when history is")
    history === nothing || (length(history) == length(planes) && length(moments) == 2 * width * height) || error("TraceHIP: history must have the size of planes, moments 2 floats per pixel")
    out, out_history = similar(xyzw), similar(planes)
    out_moments, out_variance = Array{Float32}(undef, 2, width, height), Array{Float32}(undef, width, height)
    stats = TrhipStats()
    prm = temporal_moments_params(t, history === nothing ? nothing : prev_camera)
    rc = GC.@preserve prm history moments ccall((:trhip_temporal_moments, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), moments === nothing ? Ptr{Float32}(C_NULL) : pointer(moments), width, height,
        pointer_from_objref(prm), out, out_history, out_moments, out_variance, Ref(stats))
    check(rc)
    out, out_history, out_moments, out_variance
end

# The variance-guided filter (trhip_denoise_var): `nothing` leaves a field at trhip_denoise_var_default_params'.  sigma_colour multiplies the standard deviation.
struct VarianceDenoiser
    iterations::Union{Nothing,UInt32}
    sigma_colour::Union{Nothing,Float32}
    var_eps::Union{Nothing,Float32}
    demodulate::Bool
    VarianceDenoiser(; iterations = nothing, sigma_colour = nothing, var_eps = nothing, demodulate = true) = new(iterations, sigma_colour, var_eps, demodulate)
end
function denoise_var_params(d::VarianceDenoiser)
    p = TrhipDenoiseVarParams(0, 0, 0f0, 0f0, 0f0, 0f0, 0f0, 0, 0f0, 0, (UInt32(0), UInt32(0)))
    check(ccall((:trhip_denoise_var_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    d.iterations === nothing || (p.iterations = d.iterations)
    d.sigma_colour === nothing || (p.sigma_colour = d.sigma_colour)
    d.var_eps === nothing || (p.var_eps = d.var_eps)
    p.base_flags = d.demodulate ? UInt32(1) : UInt32(0)
    p
end

# Returns (xyzw, variance of the filtered colour).
function (d::VarianceDenoiser)(xyzw::Array{Float32}, planes::Array{Float32}, variance::Array{Float32}, width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height && length(variance) == width * height ||
        error("TraceHIP: xyzw must hold 4, planes 12 and variance 1 float per pixel")
    out, out_variance = similar(xyzw), similar(variance)
    stats = TrhipStats()
    prm = denoise_var_params(d)
    rc = GC.@preserve prm ccall((:trhip_denoise_var, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, variance, width, height, pointer_from_objref(prm), out, out_variance, Ref(stats))
    check(rc)
    out, out_variance
end
