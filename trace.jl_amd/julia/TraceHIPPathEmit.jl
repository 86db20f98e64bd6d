# TraceHIPPathEmit.jl — area lights in path frames: emissive triangles (include/tracehip.h, trhip_emitters and trhip_render_path_emit; docs/design/29-path-emit.md); included
# at the end of TraceHIPPathNEE.jl, inside `module TraceHIP`, and not loadable on its own.  It uses the module's LIB, check, context, flatten, sensor, seed_of,
# shard_samples, JOB, write_film!, TrhipSensor and TrhipStats.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_path_emit_calls.json (tests/test_path_emit_api.py), as TraceHIPPathNEE.jl's are in julia_shim_path_nee_calls.json.

const TRHIP_PATH_EMIT_HITS_ONLY = UInt32(1)

# trhip_path_emit_params (32 bytes); mutable so that a Ref of it has an address the ccalls can pass as an opaque pointer
mutable struct TrhipPathEmitParams
    scale::Float32
    flags::UInt32
    reserved0::UInt32
    reserved1::UInt32
    reserved2::UInt32
    reserved3::UInt32
    reserved4::UInt32
    reserved5::UInt32
end

# The id `flatten` gives every material of the scene: in order of first appearance over the primitives, nested aggregates spliced in place.
function emit_material_ids(scene::Trace.Scene)
    ids = IdDict{Any,UInt32}()
    function walk!(list)
        for p in list
            if p isa Trace.BVHAccel
                walk!(p.primitives)
            elseif p.material !== nothing
                get!(ids, p.material, UInt32(length(ids)))
            end
        end
    end
    walk!((scene.aggregate::Trace.BVHAccel).primitives)
    ids
end

# PathIntegrator in which the triangles that carry one of `radiance`'s materials (material object => Trace.RGBSpectrum) shine on both sides: every vertex with a
# non-specular lobe casts one shadow ray towards a point drawn from them, and a path that reaches one collects its light where no such ray has accounted for it
# (hits_only = true: no shadow rays, every hit counts — plain path tracing).
struct PathEmitIntegrator <: Trace.SamplerIntegrator
    camera::Trace.Camera
    sampler::Trace.AbstractSampler
    max_depth::Int64
    radiance::Vector{Pair{Any,Trace.RGBSpectrum}}
    scale::Float32
    hits_only::Bool
    PathEmitIntegrator(camera, sampler, max_depth, radiance; scale = 1f0, hits_only = false) =
        new(camera, sampler, max_depth, collect(Pair{Any,Trace.RGBSpectrum}, radiance), scale, hits_only)
end
function path_emit_params(i::PathEmitIntegrator)
    p = TrhipPathEmitParams(0f0, 0, 0, 0, 0, 0, 0, 0)
    check(ccall((:trhip_path_emit_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.scale = i.scale
    p.flags = i.hits_only ? TRHIP_PATH_EMIT_HITS_ONLY : UInt32(0)
    p
end
# the trhip_emitters of a flattened scene: freed by the caller (trhip_emitters_free)
function emitters_handle(scene::Trace.Scene, s::Ptr{Cvoid}, radiance)
    ids = emit_material_ids(scene)
    mats = UInt32[]
    le = Float32[]
    for (m, c) in radiance
        haskey(ids, m) || error("TraceHIP: the scene has no primitive with this material")
        push!(mats, ids[m])
        append!(le, Float32[c.c...])
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:trhip_emitters_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Float32}, UInt32, Ptr{Ptr{Cvoid}}), context(), s, mats, le, length(mats), h))
    h[]
end
function emitters_size(em::Ptr{Cvoid})
    n = Ref{UInt32}(0)
    check(ccall((:trhip_emitters_size, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt32}), em, n))
    Int(n[])
end
function (i::PathEmitIntegrator)(scene::Trace.Scene)
    film = Trace.get_film(i.camera)
    s = flatten(scene)
    em = try
        emitters_handle(scene, s, i.radiance)
    catch
        ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
        rethrow()
    end
    sn = Ref(sensor(i.camera))
    h, w = size(film.pixels)
    out = Vector{Float32}(undef, 4 * h * w)
    stats = TrhipStats()
    prm = path_emit_params(i)
    seed, offset = seed_of(i.sampler)
    rank, world = JOB[]
    spp, first = world > 1 ? shard_samples(i.sampler.samples_per_pixel) : (i.sampler.samples_per_pixel, 0)
    rc = GC.@preserve prm begin
        if world > 1  # as PathNEEIntegrator: a device-resident film of this rank's shard (films are additive over sample_offset), summed over the ranks by the library
            d_film = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:hipMalloc, "libamdhip64"), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), d_film, sizeof(out)))
            r = ccall((:trhip_render_path_emit_device, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, Cint, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipStats}),
                context(), s, sn, max(spp, 1), i.max_depth, seed, offset + first, em, pointer_from_objref(prm), d_film[], Ref(stats))
            r == 0 && spp == 0 && ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0, sizeof(out))
            r == 0 || ccall((:hipMemset, "libamdhip64"), Cint, (Ptr{Cvoid}, Cint, Csize_t), d_film[], 0xff, sizeof(out))
            r_red = ccall((:trhip_film_reduce, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Cint), context(), d_film[], h * w, 0)
            r == 0 && (r = r_red)
            r == 0 && rank == 0 && ccall((:hipMemcpy, "libamdhip64"), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), out, d_film[], sizeof(out), 2)
            ccall((:hipFree, "libamdhip64"), Cint, (Ptr{Cvoid},), d_film[])
            r
        else
            ccall((:trhip_render_path_emit, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, Cint, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{TrhipStats}),
                context(), s, sn, spp, i.max_depth, seed, offset, em, pointer_from_objref(prm), out, Ref(stats))
        end
    end
    ccall((:trhip_emitters_free, LIB), Cvoid, (Ptr{Cvoid},), em)
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    rank == 0 || return nothing
    world > 1 && isnan(out[4]) && error("TraceHIP: a rank of the job failed to render its samples (the reduced film is NaN)")
    write_film!(film, out, h, w)
    Trace.save(film)
end

# (Lh.rgb, counted hits) of this process's last PathEmitIntegrator frame, 4 x n_samples, for the n_samples the frame drew
function last_emitted(n_samples::Integer)
    out = Matrix{Float32}(undef, 4, n_samples)
    check(ccall((:trhip_last_emitted, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt64), context(), out, length(out)))
    out
end
