# TraceHIPAO.jl — the ambient-occlusion part of the shim; included by TraceHIP.jl inside `module TraceHIP`, after PathIntegrator, and not loadable on its own.
# It uses the module's LIB, check, context, flatten, sensor, seed_of, shard_samples, JOB, write_film!, TrhipSensor and TrhipStats.  Its ccalls are checked against
# include/tracehip.h and written down in tests/golden/julia_shim_ao_calls.json (tests/test_julia_shim_ao.py), as TraceHIP.jl's own are in julia_shim_calls.json.

# trhip_ao_params (16 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipAoParams
    max_distance::Float32
    background::Float32
    flags::UInt32
    reserved::UInt32
end
const TRHIP_AO_ALBEDO = UInt32(1)

# Ambient occlusion (include/tracehip.h, trhip_render_ao): the camera samples of PathIntegrator, one cosine-distributed occlusion ray of reach `max_distance` per first hit,
# 1 where it escapes and 0 where it is stopped (times the base colour with `albedo`), `background` on a miss.  No lights and no materials needed.
struct AmbientOcclusionIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    max_distance::Float32
    albedo::Bool
    background::Float32
    AmbientOcclusionIntegrator(camera, sampler; max_distance = Inf32, albedo = false, background = 0f0) = new(camera, sampler, max_distance, albedo, background)
end
function ao_params(i::AmbientOcclusionIntegrator)
    p = TrhipAoParams(0f0, 0f0, 0, 0)
    check(ccall((:trhip_ao_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.max_distance, p.background, p.flags = i.max_distance, i.background, i.albedo ? TRHIP_AO_ALBEDO : UInt32(0)
    p
end
function (i::AmbientOcclusionIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    s = flatten(scene)
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = ao_params(i)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as render!: a device-resident film of this rank's shard, summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_ao_device, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipStats}),
                context(), s, sn, max(spp, 1), seed, offset + first, pointer_from_objref(prm), d_film[], Ref(stats))
            r == 0 && spp == 0 && ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0, sizeof(out))
            r == 0 || ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0xff, sizeof(out))
            r_red = ccall((:trhip_film_reduce, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Cint), context(), d_film[], h * w, 0)
            r == 0 && (r = r_red)
            r == 0 && rank == 0 && ccall((:hipMemcpy, "libamdhip64"), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), out, d_film[], sizeof(out), 2)
            ccall((:hipFree, "libamdhip64"), Cint, (Ptr{Cvoid},), d_film[])
            r
        else
            ccall((:trhip_render_ao, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, UInt64, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{TrhipStats}),
                context(), s, sn, spp, seed, offset, pointer_from_objref(prm), out, Ref(stats))
        end
    end
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    rank == 0 || return nothing
    world > 1 && isnan(out[4]) && error("TraceHIP: a rank of the job failed to render its samples (the reduced film is NaN)")
    write_film!(film, out, h, w)
    Trace.save(film)
end
