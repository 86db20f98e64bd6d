# TraceHIPPathEnv.jl — the environment term of path frames (include/tracehip.h, trhip_render_path_env; docs/design/26-path-env.md); included at the end of TraceHIPSky.jl,
# whose Environment and env_handle it uses, inside `module TraceHIP`, and not loadable on its own.  It also uses the module's LIB, check, context, flatten, sensor, seed_of,
# shard_samples, JOB, write_film!, TrhipSensor and TrhipStats.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_path_env_calls.json (tests/test_path_env_api.py), as TraceHIPSky.jl's are in julia_shim_sky_calls.json.

# trhip_path_env_params (16 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipPathEnvParams
    scale::Float32
    flags::UInt32
    reserved0::UInt32
    reserved1::UInt32
end
const TRHIP_PATH_ENV_HIDE_BACKGROUND = UInt32(1)

# PathIntegrator whose escaping paths bring back the environment's radiance: L' = L + beta * (E(dir) * scale); with `hide_background` not at depth 1 (a camera ray
# that misses stays black).  No importance sampling of the map: a small bright sun stays noisy on matte surfaces.
struct PathEnvIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    max_depth::Int64
    environment::Environment
    scale::Float32
    hide_background::Bool
    PathEnvIntegrator(camera, sampler, max_depth, environment; scale = 1f0, hide_background = false) = new(camera, sampler, max_depth, environment, scale, hide_background)
end
function path_env_params(scale, hide_background)
    p = TrhipPathEnvParams(0f0, 0, 0, 0)
    check(ccall((:trhip_path_env_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.scale = Float32(scale)
    p.flags = hide_background ? TRHIP_PATH_ENV_HIDE_BACKGROUND : UInt32(0)
    p
end
function (i::PathEnvIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    env = env_handle(i.environment)  # first: a map the library refuses throws here, before anything else is held
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = path_env_params(i.scale, i.hide_background)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as SkyIntegrator: a device-resident film of this rank's shard (films are additive over sample_offset), summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_path_env_device, LIB), Cint,
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
            ccall((:trhip_render_path_env, LIB), Cint,
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

# The escape records of this process's last path-env frame (trhip_last_escapes): 8 x n_samples — beta.xyz, the escape depth (0: none), dir.xyz, 0 — for the
# n_samples = spp * sample pixels the frame drew, indexed like the per-sample radiance.
function last_escapes(n_samples::Integer)
    out = Matrix{Float32}(undef, 8, n_samples)
    check(ccall((:trhip_last_escapes, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt64), context(), out, UInt64(length(out))))
    out
end

# The film of this process's last path-env frame under another environment and / or other parameters, without tracing a ray (trhip_path_env_relight): written into the
# camera's film.  Valid only while that frame is the context's last render.
function relight!(i::PathEnvIntegrator, environment::Environment; scale = i.scale, hide_background = i.hide_background)
    film = Trace.get_film(i.camera)
    env = env_handle(environment)
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    prm = path_env_params(scale, hide_background)
    rc = GC.@preserve prm ccall((:trhip_path_env_relight, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}), context(), env, pointer_from_objref(prm), out)
    ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), env)
    check(rc)
    write_film!(film, out, h, w)
    Trace.save(film)
end

# importance sampling of the map and the importance-sampled sky frame (trhip_render_sky_is): env_sample, env_pdf, SkyISIntegrator (tests/golden/julia_shim_sky_is_calls.json)
include("TraceHIPSkyIS.jl")
