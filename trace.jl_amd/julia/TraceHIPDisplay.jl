# TraceHIPDisplay.jl — the display pass: metered exposure, tone curve and 8-bit encode of a film on the device; included by TraceHIP.jl inside `module TraceHIP`, after
# TraceHIPUpscale.jl, and not loadable on its own.  It uses the module's LIB, check, context and TrhipStats.  Its ccalls are checked against include/tracehip.h and written
# down in tests/golden/julia_shim_display_calls.json (tests/test_julia_shim_display.py).

# trhip_display_params (48 bytes)
mutable struct TrhipDisplayParams
    curve::UInt32
    transfer::UInt32
    flags::UInt32
    exposure::Float32
    key::Float32
    percentile_permille::UInt32
    adapt_rate::Float32
    min_exposure::Float32
    max_exposure::Float32
    white::Float32
    reserved::NTuple{2,UInt32}
end

# trhip_display_state (16 bytes); all zero = no state
mutable struct TrhipDisplayState
    exposure::Float32
    valid::UInt32
    counted::UInt32
    key_bin::UInt32
end
TrhipDisplayState() = TrhipDisplayState(0f0, 0, 0, 0)

const DISPLAY_CURVES = Dict(:clamp => UInt32(0), :reinhard => UInt32(1), :aces => UInt32(2))  # TRHIP_DISPLAY_CURVE_*
const DISPLAY_TRANSFERS = Dict(:linear => UInt32(0), :srgb => UInt32(1))                     # TRHIP_DISPLAY_TRANSFER_*

# `nothing` leaves a field at trhip_display_default_params'.
struct Display
    curve::Union{Nothing,Symbol}
    transfer::Union{Nothing,Symbol}
    auto_exposure::Union{Nothing,Bool}
    flip_rows::Union{Nothing,Bool}
    exposure::Union{Nothing,Float32}
    key::Union{Nothing,Float32}
    percentile::Union{Nothing,Float64}
    adapt_rate::Union{Nothing,Float32}
    min_exposure::Union{Nothing,Float32}
    max_exposure::Union{Nothing,Float32}
    white::Union{Nothing,Float32}
    Display(; curve = nothing, transfer = nothing, auto_exposure = nothing, flip_rows = nothing, exposure = nothing, key = nothing, percentile = nothing, adapt_rate = nothing,
            min_exposure = nothing, max_exposure = nothing, white = nothing) =
        new(curve, transfer, auto_exposure, flip_rows, exposure, key, percentile, adapt_rate, min_exposure, max_exposure, white)
end
# the look of save(film): linear clamp, no transfer function, exposure 1, rows flipped
reference_display() = Display(curve = :clamp, transfer = :linear, auto_exposure = false, flip_rows = true, exposure = 1f0)

function display_params(d::Display)
    p = TrhipDisplayParams(0, 0, 0, 0f0, 0f0, 0, 0f0, 0f0, 0f0, 0f0, (UInt32(0), UInt32(0)))
    check(ccall((:trhip_display_default_params, LIB), Cint, (Ptr{Cvoid},), pointer_from_objref(p)))
    d.curve === nothing || (p.curve = DISPLAY_CURVES[d.curve])
    d.transfer === nothing || (p.transfer = DISPLAY_TRANSFERS[d.transfer])
    d.auto_exposure === nothing || (p.flags = d.auto_exposure ? (p.flags | UInt32(1)) : (p.flags & ~UInt32(1)))  # TRHIP_DISPLAY_AUTO_EXPOSURE
    d.flip_rows === nothing || (p.flags = d.flip_rows ? (p.flags | UInt32(2)) : (p.flags & ~UInt32(2)))          # TRHIP_DISPLAY_FLIP_ROWS
    d.exposure === nothing || (p.exposure = d.exposure)
    d.key === nothing || (p.key = d.key)
    d.percentile === nothing || (p.percentile_permille = UInt32(round(Int, d.percentile * 1000)))
    d.adapt_rate === nothing || (p.adapt_rate = d.adapt_rate)
    d.min_exposure === nothing || (p.min_exposure = d.min_exposure)
    d.max_exposure === nothing || (p.max_exposure = d.max_exposure)
    d.white === nothing || (p.white = d.white)
    p
end

# The 256 Float32 of the sRGB encode: [1] = 0, [k + 1] = T[k].  No context, no GPU.
function srgb_table()
    t = Vector{Float32}(undef, 256)
    check(ccall((:trhip_display_srgb_table, LIB), Cint, (Ptr{Float32},), t))
    t
end

# xyzw 4 x w x h Float32 -> (rgba 4 x w x h UInt8, histogram of 256 UInt32).  `state` (a TrhipDisplayState carried from frame to frame, or nothing) is updated in place.
function (d::Display)(xyzw::Array{Float32}, width::Integer, height::Integer, scale::Real = 1f0; state::Union{Nothing,TrhipDisplayState} = nothing)
    length(xyzw) == 4 * width * height || error("TraceHIP: xyzw must hold 4 floats per pixel")
    out, hist = Array{UInt8}(undef, 4, width, height), Vector{UInt32}(undef, 256)
    stats = TrhipStats()
    prm = display_params(d)
    rc = GC.@preserve prm state ccall((:trhip_display, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, UInt32, UInt32, Float32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt32}, Ptr{TrhipStats}),
        context(), xyzw, width, height, Float32(scale), pointer_from_objref(prm), state === nothing ? C_NULL : pointer_from_objref(state), out, hist, Ref(stats))
    check(rc)
    out, hist
end
