# TraceHIPAdaptive.jl — adaptive sampling: path frames from a per-pixel sample count, and the map made from a pilot frame; included by TraceHIP.jl inside
# `module TraceHIP`, after TraceHIPDirectSplit.jl, and not loadable on its own.  It uses the module's LIB, check, context, flatten, sensor, seed_of, write_film!, TrhipSensor and
# TrhipStats.  docs/design/24-adaptive.md is the specification.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_adaptive_calls.json (tests/test_julia_shim_adaptive.py).

# trhip_sample_map_params (24 bytes)
mutable struct TrhipSampleMapParams
    tau::Float32
    eps::Float32
    pilot::UInt32
    max_extra::UInt32
    flags::UInt32
    reserved::UInt32
end

# The library's defaults (trhip_sample_map_default_params; no context, no GPU)
function sample_map_default_params()
    p = TrhipSampleMapParams(0f0, 0f0, 0, 0, 0, 0)
    check(ccall((:trhip_sample_map_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p
end

# (sb_width, sb_height) of a film's sample bounds, filter border included: the shape of a map
function sample_bounds_size(film)
    sb = Trace.get_sample_bounds(film)
    Int(sb.p_max[1] - sb.p_min[1]) + 1, Int(sb.p_max[2] - sb.p_min[2]) + 1
end

# A path frame in which sample pixel p draws counts[p] samples (trhip_render_path_map): counts holds one UInt32 per sample pixel, rows of sb_width, each in 0:max_spp.
# Returns (xyzw, stats); the film is not written.
function render_path_map(i, scene::Trace.Scene, counts::Vector{UInt32}, max_spp::Integer; sample_offset::Integer = 0)
    film = Trace.get_film(i.camera)
    sbw, sbh = sample_bounds_size(film)
    length(counts) == sbw * sbh || error("TraceHIP: counts must hold one entry per sample pixel ($sbw x $sbh)")
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    seed, offset = seed_of(i.sampler)
    rc = ccall((:trhip_render_path_map, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, Ptr{UInt32}, UInt32, Cint, UInt64, UInt32, Ptr{Float32}, Ptr{TrhipStats}),
        context(), s, sn, counts, max_spp, i.max_depth, seed, offset + sample_offset, out, Ref(stats))
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    out, stats
end

# (m, v) of every sample pixel's luminance over the records of the context's last path frame (trhip_last_sample_stats): 2 floats per sample pixel
function last_sample_stats(n_sample_pixels::Integer)
    mv = Vector{Float32}(undef, 2 * n_sample_pixels)
    check(ccall((:trhip_last_sample_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), context(), mv))
    mv
end

# The extra samples per sample pixel (trhip_sample_map): returns (counts, their sum)
function sample_map(mv::Vector{Float32}, sb_width::Integer, sb_height::Integer, prm::TrhipSampleMapParams)
    length(mv) == 2 * sb_width * sb_height || error("TraceHIP: mv must hold 2 floats per sample pixel")
    counts = Vector{UInt32}(undef, sb_width * sb_height)
    total = Ref{UInt64}(0)
    rc = GC.@preserve prm ccall((:trhip_sample_map, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Cvoid}),
        context(), mv, sb_width, sb_height, pointer_from_objref(prm), counts, total)
    check(rc)
    counts, total[]
end

# a + b on all four lanes (trhip_film_sum): a pilot film and the map frame's film, weight lane included
function film_sum(a::Array{Float32}, b::Array{Float32}, width::Integer, height::Integer)
    length(a) == 4 * width * height && length(b) == length(a) || error("TraceHIP: both films must hold 4 floats per pixel")
    out = similar(a)
    check(ccall((:trhip_film_sum, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Float32}), context(), a, b, width, height, out))
    out
end

# A pilot frame at sampler.samples_per_pixel >= 2, the map from its records, the map frame behind the pilot's sample indices, and the sum of the two films.
# `nothing` leaves a field at trhip_sample_map_default_params'.
struct AdaptivePathIntegrator
    camera
    sampler
    max_depth::Int
    tau::Union{Nothing,Float32}
    max_extra::Union{Nothing,UInt32}
    eps::Union{Nothing,Float32}
end
AdaptivePathIntegrator(camera, sampler, max_depth; tau = nothing, max_extra = nothing, eps = nothing) = AdaptivePathIntegrator(camera, sampler, max_depth, tau, max_extra, eps)

function sample_map_params(i::AdaptivePathIntegrator)
    p = sample_map_default_params()
    p.pilot = i.sampler.samples_per_pixel
    i.tau === nothing || (p.tau = i.tau)
    i.max_extra === nothing || (p.max_extra = i.max_extra)
    i.eps === nothing || (p.eps = i.eps)
    p
end

function (i::AdaptivePathIntegrator)(scene::Trace.Scene)
    n0 = i.sampler.samples_per_pixel
    n0 >= 2 || error("TraceHIP: the pilot frame needs at least 2 samples per pixel")
    film = Trace.get_film(i.camera)
    sbw, sbh = sample_bounds_size(film)
    h, w = size(film.pixels)
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    pilot = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    seed, offset = seed_of(i.sampler)
    rc = ccall((:trhip_render_path, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, Cint, UInt64, UInt32, Ptr{Float32}, Ptr{TrhipStats}),
        context(), s, sn, n0, i.max_depth, seed, offset, pilot, Ref(stats))
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    prm = sample_map_params(i)
    counts, total = sample_map(last_sample_stats(sbw * sbh), sbw, sbh, prm)
    out = pilot
    if total > 0
        extra, _ = render_path_map(i, scene, counts, prm.max_extra; sample_offset = n0)
        out = film_sum(pilot, extra, w, h)
    end
    write_film!(film, out, h, w)
    Trace.save(film)
end
