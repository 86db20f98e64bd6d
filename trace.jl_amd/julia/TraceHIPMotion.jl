# TraceHIPMotion.jl — moving geometry in a preview: the id plane and motion-aware temporal reprojection; included by TraceHIP.jl inside `module TraceHIP`, after
# TraceHIPTemporalUpsample.jl, and not loadable on its own.  It uses the module's LIB, check, context, flatten, sensor, seed_of, TrhipSensor and TrhipStats, and
# TemporalAccumulator, temporal_params of TraceHIPTemporal.jl.  Its ccalls are checked against include/tracehip.h and written down in
# tests/golden/julia_shim_motion_calls.json (tests/test_julia_shim_motion.py).

# trhip_aov_id (16 bytes): per film pixel the nearest of its own camera samples.  prim is the ordered-primitive slot, 0-based, -1 without a hit
struct TrhipAovId
    prim::Int32
    material::Int32
    t::Float32
    n_hit::UInt32
end

# trhip_temporal_motion_params (80 bytes): trhip_temporal_params' fields, then the sizes of the body table and the matrices
mutable struct TrhipTemporalMotionParams
    prev_world_to_pixel::NTuple{12,Float32}
    max_history::Float32
    sigma_normal::Float32
    sigma_plane::Float32
    min_coverage::Float32
    n_prims::UInt32
    n_bodies::UInt32
    flags::UInt32
    reserved::UInt32
end
const STATIC_BODY = 0xffffffff  # the conventional word of body_of_prim for a primitive of no body

# The id plane of a frame (include/tracehip.h, trhip_render_aov_ids): w x h records, the camera samples those of PathIntegrator for the same camera and sampler.
function aov_ids(camera::Trace.Camera, sampler::Trace.AbstractSampler, scene::Trace.Scene)
    film = Trace.get_film(camera)
    s = flatten(scene)
    sn = Ref(sensor(camera))
    h, w = size(film.pixels)
    ids = Array{TrhipAovId}(undef, w, h)
    stats = TrhipStats()
    seed, offset = seed_of(sampler)
    rc = ccall((:trhip_render_aov_ids, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipSensor}, UInt32, UInt64, UInt32, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{TrhipStats}),
        context(), s, sn, sampler.samples_per_pixel, seed, offset, Ptr{Float32}(C_NULL), C_NULL, ids, Ref(stats))
    ccall((:trhip_scene_free, LIB), Cvoid, (Ptr{Cvoid},), s)
    check(rc)
    ids
end

# prev_from_cur of a body that `motion` (a Trace.Transformation) carried from the previous frame's pose to this one: the first three rows of its inverse, row-major
prev_from_cur(motion) = NTuple{12,Float32}(Float32(motion.inv_m[i, j]) for i in 1:3 for j in 1:4)

function temporal_motion_params(t::TemporalAccumulator, prev_camera, n_prims::Integer, n_bodies::Integer)
    p = TrhipTemporalMotionParams(ntuple(_ -> 0f0, 12), 0f0, 0f0, 0f0, 0f0, 0, 0, 0, 0)
    check(ccall((:trhip_temporal_motion_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    t.max_history === nothing || (p.max_history = t.max_history)
    t.sigma_normal === nothing || (p.sigma_normal = t.sigma_normal)
    t.sigma_plane === nothing || (p.sigma_plane = t.sigma_plane)
    t.min_coverage === nothing || (p.min_coverage = t.min_coverage)
    prev_camera === nothing || (p.prev_world_to_pixel = world_to_pixel(prev_camera))
    p.n_prims, p.n_bodies = n_prims, n_bodies
    p
end

# TemporalAccumulator's call for a scene whose rigid bodies moved (trhip_temporal_motion; docs/design/20-motion.md).  xyzw, planes, history as there; ids: this frame's
# aov_ids; body_of_prim: one UInt32 per ordered-primitive slot (STATIC_BODY: no body) or `nothing`; bodies: one prev_from_cur per body or `nothing`.  Returns (xyzw, history).
function accumulate_motion(t::TemporalAccumulator, xyzw::Array{Float32}, planes::Array{Float32}, history::Union{Nothing,Array{Float32}}, ids::Array{TrhipAovId},
                           body_of_prim::Union{Nothing,Vector{UInt32}}, bodies::Union{Nothing,Vector{NTuple{12,Float32}}}, prev_camera, width::Integer, height::Integer)
    length(xyzw) == 4 * width * height && length(planes) == 12 * width * height && length(ids) == width * height ||
        error("TraceHIP: xyzw must hold 4 and planes 12 floats per pixel, ids one record")
    history === nothing || length(history) == length(planes) || error("TraceHIP: history must have the size of planes")
    out, out_history = similar(xyzw), similar(planes)
    stats = TrhipStats()
    prm = temporal_motion_params(t, history === nothing ? nothing : prev_camera, body_of_prim === nothing ? 0 : length(body_of_prim), bodies === nothing ? 0 : length(bodies))
    rc = GC.@preserve prm history body_of_prim bodies ccall((:trhip_temporal_motion, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{UInt32}, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{TrhipStats}),
        context(), xyzw, planes, history === nothing ? Ptr{Float32}(C_NULL) : pointer(history), ids, body_of_prim === nothing ? Ptr{UInt32}(C_NULL) : pointer(body_of_prim),
        bodies === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(bodies)), width, height, pointer_from_objref(prm), out, out_history, Ref(stats))
    check(rc)
    out, out_history
end
