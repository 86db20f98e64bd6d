# TraceHIPSkyIS.jl — importance sampling of the environment map and the importance-sampled sky frame (include/tracehip.h, trhip_env_make_sampler, trhip_render_sky_is;
# docs/design/27-sky-importance.md); included at the end of TraceHIPPathEnv.jl, after TraceHIPSky.jl's Environment, env_handle and the two sky flags, which it uses, inside
# `module TraceHIP`, and not loadable on its own.  It also uses the module's LIB, check, context, flatten, sensor, seed_of, shard_samples, JOB, write_film!, TrhipSensor and
# TrhipStats.  Its ccalls are checked against include/tracehip.h and written down in tests/golden/julia_shim_sky_is_calls.json (tests/test_sky_is_api.py), as
# TraceHIPPathEnv.jl's are in julia_shim_path_env_calls.json.

# trhip_sky_is_params (32 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipSkyIsParams
    max_distance::Float32
    scale::Float32
    mix::Float32
    flags::UInt32
    reserved0::UInt32
    reserved1::UInt32
    reserved2::UInt32
    reserved3::UInt32
end

# the device copy of `e` with its sampling tables; the caller frees it with trhip_env_free.  A matrix that is not orthonormal and a black map throw here.
function env_sampler_handle(e::Environment)
    h = env_handle(e)
    rc = ccall((:trhip_env_make_sampler, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), context(), h)
    rc == 0 || ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    check(rc)
    h
end

# a unit direction for every point of `u` (2 x count, in [0, 1)^2), distributed like the map's radiance times solid angle: the device's deterministic sampler
function env_sample(e::Environment, u::AbstractMatrix{<:Real})
    size(u, 1) == 2 || error("TraceHIP: sample points must be 2 x count")
    p = Matrix{Float32}(u)
    out = Matrix{Float32}(undef, 3, size(p, 2))
    h = env_sampler_handle(e)
    rc = ccall((:trhip_env_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, UInt64, Ptr{Float32}), context(), h, p, UInt64(size(p, 2)), out)
    ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    check(rc)
    out
end

# the density, with respect to solid angle, with which env_sample returns the directions `dirs` (3 x count)
function env_pdf(e::Environment, dirs::AbstractMatrix{<:Real})
    size(dirs, 1) == 3 || error("TraceHIP: directions must be 3 x count")
    d = Matrix{Float32}(dirs)
    out = Vector{Float32}(undef, size(d, 2))
    h = env_sampler_handle(e)
    rc = ccall((:trhip_env_pdf, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, UInt64, Ptr{Float32}), context(), h, d, UInt64(size(d, 2)), out)
    ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    check(rc)
    out
end

# SkyIntegrator whose occlusion rays are drawn from the map's own distribution with probability `mix`, weighted as the one-sample mixture estimator does
# (trhip_render_sky_is): unbiased as the sky frame, far less noise under a small bright sun.
struct SkyISIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    environment::Environment
    max_distance::Float32
    albedo::Bool
    scale::Float32
    hide_background::Bool
    mix::Float32
    SkyISIntegrator(camera, sampler, environment; max_distance = Inf32, albedo = false, scale = 1f0, hide_background = false, mix = 0.5f0) =
        new(camera, sampler, environment, max_distance, albedo, scale, hide_background, mix)
end
function sky_is_params(i::SkyISIntegrator)
    p = TrhipSkyIsParams(0f0, 0f0, 0f0, 0, 0, 0, 0, 0)
    check(ccall((:trhip_sky_is_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.max_distance, p.scale, p.mix = i.max_distance, i.scale, i.mix
    p.flags = (i.albedo ? TRHIP_SKY_ALBEDO : UInt32(0)) | (i.hide_background ? TRHIP_SKY_HIDE_BACKGROUND : UInt32(0))
    p
end
function (i::SkyISIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    env = env_sampler_handle(i.environment)  # first: a map the library refuses throws here, before anything else is held
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = sky_is_params(i)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as SkyIntegrator: a device-resident film of this rank's shard (films are additive over sample_offset), summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_sky_is_device, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipStats}),
                context(), s, sn, max(spp, 1), seed, offset + first, env, pointer_from_objref(prm), d_film[], Ref(stats))
            r == 0 && spp == 0 && ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0, sizeof(out))
            r == 0 || ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0xff, sizeof(out))
            r_red = ccall((:trhip_film_reduce, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Cint), context(), d_film[], h * w, 0)
            r == 0 && (r = r_red)
            r == 0 && rank == 0 && ccall((:hipMemcpy, "libamdhip64"), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), out, d_film[], sizeof(out), 2)
            ccall((:hipFree, "libamdhip64"), Cint, (Ptr{Cvoid},), d_film[])
            r
        else
            ccall((:trhip_render_sky_is, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{TrhipStats}),
                context(), s, sn, spp, seed, offset, env, pointer_from_objref(prm), out, Ref(stats))
        end
    end
    ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), env)
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    rank == 0 || return nothing
    world > 1 && isnan(out[4]) && error("TraceHIP: a rank of the job failed to render its samples (the reduced film is NaN)")
    write_film!(film, out, h, w)
    Trace.save(film)
end

# next-event estimation of the environment map in path frames (trhip_render_path_env_nee): PathNEEIntegrator (tests/golden/julia_shim_path_nee_calls.json)
include("TraceHIPPathNEE.jl")
