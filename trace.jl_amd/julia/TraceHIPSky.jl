# TraceHIPSky.jl — the environment map and the sky-lit frame; included by TraceHIP.jl inside `module TraceHIP`, after the other frames' files, and not loadable on its own.
# It uses the module's LIB, check, context, flatten, sensor, seed_of, shard_samples, JOB, write_film!, TrhipSensor and TrhipStats.  Its ccalls are checked against
# include/tracehip.h and written down in tests/golden/julia_shim_sky_calls.json (tests/test_sky_api.py), as TraceHIPAO.jl's are in julia_shim_ao_calls.json.

# trhip_sky_params (16 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipSkyParams
    max_distance::Float32
    scale::Float32
    flags::UInt32
    reserved::UInt32
end
const TRHIP_SKY_ALBEDO = UInt32(1)
const TRHIP_SKY_HIDE_BACKGROUND = UInt32(2)

# An environment E(w) (include/tracehip.h, trhip_env): an octahedral map of n x n RGB texels, finite and >= 0.
#   texels        3 x n x n, (channel, column i, row j): in memory the C layout n x n x 3, row j, column i
#   world_to_env  3 x 3 as Julia holds a matrix (column-major); the library takes it row-major, so its transpose is passed
struct Environment
    texels::Array{Float32, 3}
    world_to_env::Matrix{Float32}
    function Environment(texels::AbstractArray{<:Real, 3}, world_to_env::AbstractMatrix{<:Real} = Float32[1 0 0; 0 1 0; 0 0 1])
        size(texels, 1) == 3 && size(texels, 2) == size(texels, 3) || error("TraceHIP: Environment texels must be 3 x n x n")
        size(world_to_env) == (3, 3) || error("TraceHIP: Environment world_to_env must be 3 x 3")
        new(Array{Float32, 3}(texels), Matrix{Float32}(world_to_env))
    end
end
# the same radiance from every direction: one texel
constant_environment(rgb) = Environment(reshape(Float32[rgb[1], rgb[2], rgb[3]], 3, 1, 1))

# the device copy of `e` on this process's context; the caller frees it with trhip_env_free
function env_handle(e::Environment)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    r = Matrix{Float32}(permutedims(e.world_to_env))
    check(ccall((:trhip_env_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt32, Ptr{Float32}, Ptr{Ptr{Cvoid}}), context(), e.texels, UInt32(size(e.texels, 2)), r, h))
    h[]
end

# E(w) for the directions `dirs` (3 x count), evaluated on the device by the lookup the sky frame uses
function env_eval(e::Environment, dirs::AbstractMatrix{<:Real})
    size(dirs, 1) == 3 || error("TraceHIP: directions must be 3 x count")
    d = Matrix{Float32}(dirs)
    out = similar(d)
    h = env_handle(e)
    rc = ccall((:trhip_env_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, UInt64, Ptr{Float32}), context(), h, d, UInt64(size(d, 2)), out)
    ccall((:trhip_env_free, LIB), Cvoid, (Ptr{Cvoid},), h)
    check(rc)
    out
end

# A sky-lit frame (include/tracehip.h, trhip_render_sky): AmbientOcclusionIntegrator's frame in which the occlusion ray that escapes brings back the environment's radiance
# from its direction, times `scale` (times the base colour with `albedo`), and a camera ray that misses shows the environment (0 with `hide_background`).
struct SkyIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    environment::Environment
    max_distance::Float32
    albedo::Bool
    scale::Float32
    hide_background::Bool
    SkyIntegrator(camera, sampler, environment; max_distance = Inf32, albedo = false, scale = 1f0, hide_background = false) =
        new(camera, sampler, environment, max_distance, albedo, scale, hide_background)
end
function sky_params(i::SkyIntegrator)
    p = TrhipSkyParams(0f0, 0f0, 0, 0)
    check(ccall((:trhip_sky_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.max_distance, p.scale = i.max_distance, i.scale
    p.flags = (i.albedo ? TRHIP_SKY_ALBEDO : UInt32(0)) | (i.hide_background ? TRHIP_SKY_HIDE_BACKGROUND : UInt32(0))
    p
end
function (i::SkyIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    env = env_handle(i.environment)  # first: a map the library refuses throws here, before anything else is held
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = sky_params(i)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as AmbientOcclusionIntegrator: a device-resident film of this rank's shard, summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_sky_device, LIB), Cint,
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
            ccall((:trhip_render_sky, LIB), Cint,
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

# the environment term of path frames (trhip_render_path_env): PathEnvIntegrator, last_escapes, relight! (tests/golden/julia_shim_path_env_calls.json)
include("TraceHIPPathEnv.jl")
