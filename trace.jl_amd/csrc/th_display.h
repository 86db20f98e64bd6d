// th_display.h — the display pass: meter the film's luminance, resolve an exposure, apply a tone curve and encode to 8-bit RGBA (include/tracehip.h, trhip_display; the
// arithmetic is specified in docs/design/18-display.md and every line below is one Float32 operation of that text).  No transcendental: luminance is the film's .y lane,
// metering is an integer histogram of Float32 exponent bits (order-free: the atomics cannot change a bit), the sRGB encode is a search in the 255 thresholds of
// th_display_srgb.h.
//
//   k_display_meter     256 lanes per block, 16-byte loads, a grid-stride loop over the pixels on ONE block per CU; a 256-bin histogram per block in LDS, one LDS atomic add
//                       per counted lane, and one global add per non-empty bin at the end.  Measured at 1024^2 (profiles/r15/display.txt): the kernel's time is the
//                       global adds' — blocks x non-empty bins of them on 256 addresses — so it grows with the grid: 0.013 ms at one block per CU, 0.044 at eight, 0.060
//                       at sixteen on a path frame with 188 non-empty bins.  The wave-aggregated form (leader's bin by readlane, a ballot of the lanes holding it, one
//                       LDS add of their number, until the wave is served) gave the same counts and lost on that frame at every grid (0.062 ms at one block per CU: a
//                       wave of a real frame holds many bins, and the loop runs once per bin); it won only on a frame of one constant luminance at two blocks per CU and
//                       more, by 3 - 5 %.  It is not in the tree.
//   k_display_resolve   one wave: four bins per lane, a prefix sum across the lanes, the percentile's bin, the exposure and the new state.  A kernel of its own and not
//                       the prologue of the encode kernel: the state is updated in place, and a block writing it would race the blocks that have not read it yet.
//   k_display_encode    one pixel per lane, blocks of 16 x 16, a wave a 16 x 4 patch (the à-trous kernel's); the thresholds in LDS, an 8-step branch-free search per
//                       channel, one dword store per lane.
#pragma once
#include "th_denoise.h"
#include "th_display_srgb.h"

namespace th {

constexpr int kDisplayBins = 256;
constexpr uint32_t kDisplayBinBase = 856;  // bits(2^-20) >> 20: eight bins per octave from 2^-20 on
constexpr float kDisplayMinY = 9.5367431640625e-07f;  // 2^-20
constexpr float kDisplayMaxC = 1099511627776.0f;      // 2^40

__device__ const float d_srgb_thresholds[256] = {TH_SRGB_THRESHOLDS};

struct DisplayState {  // trhip_display_state
    float exposure;
    uint32_t valid, counted, key_bin;
};

struct DisplayResolveConst {
    float exposure, key, adapt_rate, min_exposure, max_exposure;
    uint32_t permille;
};

// M: whether pixel B is metered, and its bin.
TH_D bool display_bin(const float4& B, float scale, uint32_t& bin) {
    const float iw = 1.0f / B.w;
    float Y = B.y * iw;
    Y = Y * scale;
    const bool counted = B.w > 0.0f && Y >= kDisplayMinY && Y < kInf;
    const uint32_t b = (__builtin_bit_cast(uint32_t, Y) >> 20) - kDisplayBinBase;
    bin = b > 255u ? 255u : b;
    return counted;
}

__global__ __launch_bounds__(256) void k_display_meter(const float4* __restrict__ xyzw, uint32_t n, float scale, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kDisplayBins];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint32_t bin;
        if (display_bin(xyzw[i], scale, bin)) atomicAdd(&s_hist[bin], 1u);
    }
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// lower edge of bin b; L(256) = 2^12
TH_D float display_edge(uint32_t b) { return __builtin_bit_cast(float, (b + kDisplayBinBase) << 20); }

// R.  One wave.  `state` is read and rewritten; `out_hist` (may be null) receives the 256 counts.
__global__ __launch_bounds__(64) void k_display_resolve(const uint32_t* __restrict__ hist, DisplayResolveConst k, DisplayState* state, uint32_t* __restrict__ out_hist) {
    const uint32_t lane = threadIdx.x;
    const uint4 h4 = reinterpret_cast<const uint4*>(hist)[lane];
    const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
    if (out_hist)  // the caller's pointer: nothing is assumed of its alignment beyond a word's
        for (int j = 0; j < 4; ++j) out_hist[4 * lane + j] = h[j];
    const uint32_t own = (h[0] + h[1]) + (h[2] + h[3]);
    uint32_t incl = own;  // inclusive prefix over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    const DisplayState s = *state;
    if (total == 0) {
        if (lane == 0) {
            const float E = s.valid ? s.exposure : k.exposure;
            *state = DisplayState{E, s.valid, 0u, 0u};
        }
        return;
    }
    const uint64_t want = (uint64_t)total * k.permille;
    // the smallest bin b with cum(b) * 1000 >= total * permille: the first lane whose inclusive prefix reaches it holds that bin
    const bool reached = (uint64_t)incl * 1000u >= want;
    const uint64_t lanes = __ballot(reached);
    if (lane != (uint32_t)__builtin_ctzll(lanes)) return;
    uint32_t cum = incl - own;  // cum(b - 1) of this lane's first bin
    uint32_t b = 4 * lane, hb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hb = h[j];
        b = 4 * lane + (uint32_t)j;
        if ((uint64_t)(cum + hb) * 1000u >= want) break;
        cum += hb;
    }
    const uint32_t need = (uint32_t)((want + 999u) / 1000u);
    const float frac = (float)(need - cum) / (float)hb;
    const float L0 = display_edge(b);
    const float width = display_edge(b + 1) - L0;
    float Lm = frac * width;
    Lm = L0 + Lm;
    const float Et = jclamp(k.key / Lm, k.min_exposure, k.max_exposure);
    float E = Et;
    if (s.valid && k.adapt_rate < 1.0f) {
        float d = Et - s.exposure;
        d = d * k.adapt_rate;
        E = s.exposure + d;
    }
    *state = DisplayState{E, 1u, total, b};
}

struct DisplayEncodeConst {
    float scale;
    float exposure;  // E without AUTO
    float ww;        // white * white
    uint32_t flip;
};

// D3 + D4 for one channel
template <int CURVE>
TH_D float display_curve(float c, float ww) {
    float t = c;
    if (CURVE == 1) {
        float a = c / ww;
        a = 1.0f + a;
        a = c * a;
        t = a / (1.0f + c);
    } else if (CURVE == 2) {
        float a = 2.51f * c;
        a = a + 0.03f;
        a = c * a;
        float b = 2.43f * c;
        b = b + 0.59f;
        b = c * b;
        b = b + 0.14f;
        t = a / b;
    }
    t = t > 1.0f ? 1.0f : (t < 0.0f ? 0.0f : t);
    if (t != t) t = 0.0f;
    return t;
}

// D5
template <int TRANSFER>
TH_D uint32_t display_quantise(float t, const float* s_T) {
    if (TRANSFER == 0) return (uint32_t)(int)__builtin_rintf(t * 255.0f);
    uint32_t q = 0;  // the largest k with t >= T[k], T[0] = 0: the number of k in 1..255 with t >= T[k]
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1) q += t >= s_T[q + step] ? step : 0u;
    return q;
}

// `state` null: E is k.exposure (AUTO off).  Otherwise E is what k_display_resolve left in it.
template <int CURVE, int TRANSFER>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_display_encode(const float4* __restrict__ xyzw, int width, int height, DisplayEncodeConst k, const DisplayState* __restrict__ state,
                                                                      uint32_t* __restrict__ out) {
    __shared__ float s_T[256];
    if (TRANSFER == 1) {
        s_T[threadIdx.x] = d_srgb_thresholds[threadIdx.x];
        __syncthreads();
    }
    const int x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1)), y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= height) return;
    const int src_y = k.flip ? height - 1 - y : y;
    const float4 B = xyzw[(size_t)src_y * (size_t)width + (size_t)x];
    const float E = state ? state->exposure : k.exposure;
    // D1: k_film_to_rgb up to its last multiply
    f3 c = xyz_to_rgb(mk3(B.x, B.y, B.z));
    if (B.w != 0.0f) {
        const float iw = 1.0f / B.w;
        c = mk3(jmax(0.0f, c.x * iw), jmax(0.0f, c.y * iw), jmax(0.0f, c.z * iw));
    }
    c = c * k.scale;
    // D2
    c = c * E;
    c.x = c.x > kDisplayMaxC ? kDisplayMaxC : c.x;
    c.y = c.y > kDisplayMaxC ? kDisplayMaxC : c.y;
    c.z = c.z > kDisplayMaxC ? kDisplayMaxC : c.z;
    const uint32_t r = display_quantise<TRANSFER>(display_curve<CURVE>(c.x, k.ww), s_T);
    const uint32_t g = display_quantise<TRANSFER>(display_curve<CURVE>(c.y, k.ww), s_T);
    const uint32_t b = display_quantise<TRANSFER>(display_curve<CURVE>(c.z, k.ww), s_T);
    const uint32_t a = B.w != 0.0f ? 255u : 0u;  // D6
    out[(size_t)y * (size_t)width + (size_t)x] = r | g << 8 | b << 16 | a << 24;
}

}  // namespace th
