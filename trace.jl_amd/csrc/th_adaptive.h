// th_adaptive.h — adaptive sampling (docs/design/24-adaptive.md): what a frame with a per-pixel sample count needs beside the path kernels (th_kernels.h: the MapJobs form of k_raygen,
// the MapSpp forms of k_film_gather_packed and k_film_gather_block, k_film_positions_map), and the two kernels that make such a map from a pilot frame's radiance records.
// Every rule below is specified operation by operation; tests/sample_map_model.py is the same arithmetic in numpy and the kernels are bit-equal to it.
#pragma once
#include "th_kernels.h"

namespace th {

// ---- the map of a frame -----------------------------------------------------------------------------------------------------------------
// word[0] = Σ counts (< 2^63) | bit 63 when some count lies above max_spp: the eight bytes the _device entry point reads back to plan its batches
constexpr unsigned long long kMapAboveMax = 1ull << 63;
template <int TH_ONE_COPY = 0> __global__ __launch_bounds__(kBlock) void k_map_reduce(const uint32_t* __restrict__ counts, uint32_t npix, uint32_t max_spp, unsigned long long* __restrict__ word) {
    unsigned long long sum = 0;
    bool above = false;
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        const uint32_t c = counts[p];
        sum += c;
        above = above || c > max_spp;
    }
    sum = wave_sum(sum);
    const bool any_above = __any(above);
    if (lane_id() == 0) {
        if (sum) atomicAdd(word, sum);
        if (any_above) atomicOr(word, kMapAboveMax);
    }
}
// The job list: sample s < counts[p] of sample pixel p is job offsets[p] + s (offsets = the exclusive sum of counts), and a job's word is the sample's dense sample-major
// slot s * npix + p — what slot_info takes apart and film_index re-lays.  Jobs are pixel-major: the samples of one pixel sit side by side in a wave.
template <int TH_ONE_COPY = 0> __global__ __launch_bounds__(kBlock) void k_map_expand(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets, uint32_t npix, uint32_t* __restrict__ jobs) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        const uint32_t c = counts[p], o = offsets[p];
        for (uint32_t s = 0; s < c; ++s) jobs[o + s] = s * npix + p;
    }
}
// k_export_L for a map frame: the dense max_spp array, +0 where the sample was not drawn (its record was never written and is not read here)
template <int TH_ONE_COPY = 0> __global__ void k_export_L_map(const float4* __restrict__ L, uint64_t n, float* __restrict__ out, uint32_t layout, uint32_t npix, uint32_t spp, const uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = (uint32_t)(i / npix), pix = (uint32_t)(i % npix);
    f3 c = splat3(0.0f);
    if (s < counts[pix]) {
        const float4 l = L[film_index(layout, npix, spp, s, pix)];
        c = mk3(l.x, l.y, l.z);
        if (has_nan(c)) c = splat3(0.0f);
    }
    out[3 * i] = c.x;
    out[3 * i + 1] = c.y;
    out[3 * i + 2] = c.z;
}

// out = a + b on all four lanes, one Float32 addition each: a pilot film and a map frame's film are sums over disjoint sample sets, weight lane included
// (trhip_film_add keeps a's weight lane: it puts a direct film back onto its own remainder)
template <int TH_ONE_COPY = 0> __global__ __launch_bounds__(kBlock) void k_film_sum(const float4* a, const float4* b, uint64_t n, float4* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const float4 x = a[i], y = b[i];
        out[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
}

// ---- where a map comes from ----------------------------------------------------------------------------------------------------------------
// (m, v) of a sample pixel's luminance over the n = spp radiance records of the last path frame, either record layout:
//   per sample, in index order: the NaN rule (integrators/sampler.jl:46), Y = to_Y(l), S1 += Y, S2 += Y * Y, both from +0
//   m = S1 / n;  x = S2 / n - m * m;  v = x < 0 ? +0 : x   (a NaN x stays a NaN: the map rule below counts it as +Inf)
template <int TH_ONE_COPY = 0> __global__ __launch_bounds__(kBlock) void k_sample_stats(const float4* __restrict__ L, uint32_t layout, uint32_t npix, uint32_t spp, float2* __restrict__ out_mv) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        float s1 = 0.0f, s2 = 0.0f;
        for (uint32_t s = 0; s < spp; ++s) {
            const float4 l4 = L[film_index(layout, npix, spp, s, p)];
            f3 l = mk3(l4.x, l4.y, l4.z);
            if (has_nan(l)) l = splat3(0.0f);
            const float y = to_Y(l);
            s1 += y;
            s2 += y * y;
        }
        const float n = (float)spp;
        const float m = s1 / n;
        const float x = s2 / n - m * m;
        out_mv[p] = make_float2(m, x < 0.0f ? 0.0f : x);
    }
}
struct SampleMapRule {  // trhip_sample_map_params, checked
    float tau, eps;
    uint32_t pilot, max_extra;
};
//   e[q] = v / ((|m| + eps) * (|m| + eps)), +Inf when that is NaN or not finite
//   E[p] = the largest e over the 3 x 3 sample pixels inside the bounds, rows then columns ascending, from +0 with `e > E`
//   x = E / (tau * tau);  counts[p] = max_extra when !(x < float(pilot + max_extra)), otherwise max(0, int(ceilf(x)) - pilot)
template <int TH_ONE_COPY = 0> __global__ __launch_bounds__(kBlock) void k_sample_map(const float2* __restrict__ mv, uint32_t w, uint32_t h, SampleMapRule r, uint32_t* __restrict__ counts,
                                                       unsigned long long* __restrict__ total) {
    const uint32_t npix = w * h;
    unsigned long long sum = 0;
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npix; p += gridDim.x * kBlock) {
        const int y = (int)(p / w), x = (int)(p - (uint32_t)y * w);
        float E = 0.0f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) continue;
                const float2 q = mv[(uint32_t)qy * w + (uint32_t)qx];
                const float a = fabs_(q.x) + r.eps;
                float e = q.y / (a * a);
                if (!(fabs_(e) < __builtin_inff())) e = __builtin_inff();
                if (e > E) E = e;
            }
        const float xs = E / (r.tau * r.tau);
        uint32_t c = r.max_extra;
        if (xs < (float)(r.pilot + r.max_extra)) {
            const int need = (int)__builtin_ceilf(xs) - (int)r.pilot;
            c = need > 0 ? (uint32_t)need : 0u;
        }
        counts[p] = c;
        sum += c;
    }
    sum = wave_sum(sum);
    if (lane_id() == 0 && sum) atomicAdd(total, sum);
}

}  // namespace th
