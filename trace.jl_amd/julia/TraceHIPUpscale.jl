# TraceHIPUpscale.jl — edge-aware upscaling of a low-resolution path film onto the feature planes of the full-size sensor; included by TraceHIP.jl inside `module TraceHIP`,
# after TraceHIPVariance.jl, and not loadable on its own.  It uses the module's LIB, check, context and TrhipStats.  Its ccalls are checked against include/tracehip.h and
# written down in tests/golden/julia_shim_upscale_calls.json (tests/test_julia_shim_upscale.py).

# trhip_upscale_params (48 bytes)
mutable struct TrhipUpscaleParams
    lo_from_hi::NTuple{4,Float32}
    radius::UInt32
    flags::UInt32
    sigma_normal::Float32
    sigma_plane::Float32
    albedo_floor::Float32
    min_coverage::Float32
    reserved::NTuple{2,UInt32}
end

# (ax, bx, ay, by) of lo_from_hi for two films of one camera: array pixel x of the full-size film lies at x * ax + bx in the low film's array coordinates.  Film pixel X
# (1-based) has its centre at raster position X + 0.5 and array index X - crop_min (docs/design/14-temporal.md); the two rasters share the optical axis, which pierces them at
# o = -m[1,4] / m[1,1] of raster_to_camera (y: -m[2,4] / m[2,2]), and differ by the ratio of the resolutions about it.  Float64, rounded once (docs/design/17-upscale.md).
function pixel_map(hi_camera::Trace.PerspectiveCamera, lo_camera::Trace.PerspectiveCamera)
    hi, lo = Trace.get_film(hi_camera), Trace.get_film(lo_camera)
    mh, ml = rowmajor(hi_camera.core.raster_to_camera.m), rowmajor(lo_camera.core.raster_to_camera.m)
    m = Float32[]
    for k in 1:2
        d, t = 5 * (k - 1) + 1, 4 * k  # row-major positions of m[k,k] and m[k,4]
        o_hi, o_lo = -Float64(mh[t]) / Float64(mh[d]), -Float64(ml[t]) / Float64(ml[d])
        a = Float64(lo.resolution[k]) / Float64(hi.resolution[k])
        b = (Float64(hi.crop_bounds.p_min[k]) + 0.5 - o_hi) * a + o_lo - 0.5 - Float64(lo.crop_bounds.p_min[k])
        push!(m, Float32(a), Float32(b))
    end
    (m[1], m[2], m[3], m[4])
end

# `nothing` leaves a field at trhip_upscale_default_params'.
struct Upscaler
    radius::Union{Nothing,UInt32}
    sigma_normal::Union{Nothing,Float32}
    sigma_plane::Union{Nothing,Float32}
    demodulate::Union{Nothing,Bool}
    coverage::Union{Nothing,Bool}
    Upscaler(; radius = nothing, sigma_normal = nothing, sigma_plane = nothing, demodulate = nothing, coverage = nothing) = new(radius, sigma_normal, sigma_plane, demodulate, coverage)
end
function upscale_params(u::Upscaler, map::NTuple{4,Float32})
    p = TrhipUpscaleParams(ntuple(_ -> 0f0, 4), 0, 0, 0f0, 0f0, 0f0, 0f0, (UInt32(0), UInt32(0)))
    check(ccall((:trhip_upscale_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    p.lo_from_hi = map
    u.radius === nothing || (p.radius = u.radius)
    u.sigma_normal === nothing || (p.sigma_normal = u.sigma_normal)
    u.sigma_plane === nothing || (p.sigma_plane = u.sigma_plane)
    u.demodulate === nothing || (p.flags = u.demodulate ? (p.flags | UInt32(1)) : (p.flags & ~UInt32(1)))  # TRHIP_UPSCALE_DEMODULATE
    u.coverage === nothing || (p.flags = u.coverage ? (p.flags | UInt32(2)) : (p.flags & ~UInt32(2)))        # TRHIP_UPSCALE_COVERAGE
    p
end

# lo_xyzw 4 x lw x lh Float32, lo_planes 4 x 3 x lw x lh, hi_planes 4 x 3 x w x h.  Returns (xyzw 4 x w x h, mask w x h: 0 nothing, 1 guided, 2 unguided, 3 orphan).
function (u::Upscaler)(lo_xyzw::Array{Float32}, lo_planes::Array{Float32}, lo_width::Integer, lo_height::Integer, hi_planes::Array{Float32}, width::Integer, height::Integer,
                       map::NTuple{4,Float32})
    length(lo_xyzw) == 4 * lo_width * lo_height && length(lo_planes) == 12 * lo_width * lo_height && length(hi_planes) == 12 * width * height ||
        error("TraceHIP: lo_xyzw must hold 4, lo_planes and hi_planes 12 floats per pixel")
    out, mask = Array{Float32}(undef, 4, width, height), Array{UInt8}(undef, width, height)
    stats = TrhipStats()
    prm = upscale_params(u, map)
    rc = GC.@preserve prm ccall((:trhip_upscale, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt32, UInt32, Ptr{Float32}, UInt32, UInt32, Ptr{Cvoid}, Ptr{Float32}, Ptr{UInt8}, Ptr{TrhipStats}),
        context(), lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, width, height, pointer_from_objref(prm), out, mask, Ref(stats))
    check(rc)
    out, mask
end
