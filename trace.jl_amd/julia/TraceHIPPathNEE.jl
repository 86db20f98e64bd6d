# TraceHIPPathNEE.jl — next-event estimation of the environment map in path frames (include/tracehip.h, trhip_render_path_env_nee; docs/design/28-path-nee.md); included at
# the end of TraceHIPSkyIS.jl, after its env_sampler_handle and TraceHIPPathEnv.jl's TRHIP_PATH_ENV_HIDE_BACKGROUND and last_escapes, which it uses, inside `module TraceHIP`,
# and not loadable on its own.  It also uses the module's LIB, check, context, flatten, sensor, seed_of, shard_samples, JOB, write_film!, TrhipSensor and TrhipStats.  Its
# ccalls are checked against include/tracehip.h and written down in tests/golden/julia_shim_path_nee_calls.json (tests/test_path_nee_api.py), as TraceHIPSkyIS.jl's are in
# julia_shim_sky_is_calls.json.

# trhip_path_nee_params (32 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipPathNeeParams
    scale::Float32
    mix::Float32
    flags::UInt32
    reserved0::UInt32
    reserved1::UInt32
    reserved2::UInt32
    reserved3::UInt32
    reserved4::UInt32
end

# PathEnvIntegrator with one shadow ray towards the map at every vertex that has a non-specular lobe — drawn from the map's own distribution with probability `mix`, from
# the BSDF otherwise, weighted as the one-sample mixture estimator does — and without the escapes that follow such a vertex: the same expectation up to the depth cut, far
# less noise under a small bright sun.  last_escapes works after it (the 8th float is 1 where an escape is suppressed); relight! does not.
struct PathNEEIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    max_depth::Int64
    environment::Environment
    scale::Float32
    hide_background::Bool
    mix::Float32
    PathNEEIntegrator(camera, sampler, max_depth, environment; scale = 1f0, hide_background = false, mix = 0.5f0) =
        new(camera, sampler, max_depth, environment, scale, hide_background, mix)
end
function path_nee_params(i::PathNEEIntegrator)
    p = TrhipPathNeeParams(0f0, 0f0, 0, 0, 0, 0, 0, 0)
    check(ccall((:trhip_path_nee_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.scale, p.mix = i.scale, i.mix
    p.flags = i.hide_background ? TRHIP_PATH_ENV_HIDE_BACKGROUND : UInt32(0)
    p
end
function (i::PathNEEIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    env = env_sampler_handle(i.environment)  # first: a map the library refuses throws here, before anything else is held
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = path_nee_params(i)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as PathEnvIntegrator: a device-resident film of this rank's shard (films are additive over sample_offset), summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_path_env_nee_device, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, Cint, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipStats}),
                context(), s, sn, max(spp, 1), i.max_depth, seed, offset + first, env, pointer_from_objref(prm), d_film[], Ref(stats))
            r == 0 && spp == 0 && ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0, sizeof(out))
            r == 0 || ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0xff, sizeof(out))
            r_red = ccall((:trhip_film_reduce, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Cint), context(), d_film[], h * w, 0)
            r == 0 && (r = r_red)
            r == 0 && rank == 0 && ccall((:hipMemcpy, "libamdhip64"), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), out, d_film[], sizeof(out), 2)
            ccall((:hipFree, "libamdhip64"), Cint, (Ptr{Cvoid},), d_film[])
            r
        else
            ccall((:trhip_render_path_env_nee, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, Cint, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{TrhipStats}),
                context(), s, sn, spp, i.max_depth, seed, offset, env, pointer_from_objref(prm), out, Ref(stats))
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

# which escapes of this process's last PathNEEIntegrator frame do not count (the 8th float of trhip_last_escapes), for the n_samples the frame drew
suppressed_escapes(n_samples::Integer) = last_escapes(n_samples)[8, :] .!= 0f0

include("TraceHIPPathEmit.jl")
