// th_denoise_var.h — the à-trous filter of th_denoise.h with a per-pixel, per-iteration colour sigma from a variance plane that is filtered along (SVGF, Schied et al. 2017,
// section 4.3; include/tracehip.h, trhip_denoise_var; the arithmetic is specified in docs/design/16-variance.md and every line below is one Float32 operation of that text).
// Prepare and Finish are th_denoise.h's kernels; the guides, the colour buffers and the base colour are laid out as there.
//
//   k_denoise_var_seed         the caller's variance plane -> V_0: (v > 0) ? v : 0 at surface pixels, the sentinel -1 elsewhere
//   k_denoise_var_atrous       one iteration at step s, straight from memory: nine 4-byte loads for the 3 x 3 pre-filter, then per tap three 16-byte loads and one of 4 bytes
//   k_denoise_var_atrous_lds   steps 1 and 2: the same iteration with the block's pixels and their halo of 2 s staged in LDS first, the pre-filter read from LDS too
//   k_denoise_var_export       the last V -> the caller's plane, 0 where the sentinel stands
//
// The variance travels as one float per pixel, ping-ponged beside {c, Y}: 8 bytes per pixel more than trhip_denoise's 80.  A pixel that is no surface pixel holds -1 there, so
// the pre-filter needs no second array to know which of its nine positions count: a variance is never negative (V_0 is clamped, every later V is a quotient of sums of
// non-negative terms, and a NaN quotient is stored as 0).
#pragma once
#include "th_denoise.h"

namespace th {

constexpr float kDvNoSurface = -1.0f;

TH_D float dv_prefilter_weight(int d) { return d == 0 ? 0.5f : 0.25f; }

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_denoise_var_seed(const float4* __restrict__ gn, const float* __restrict__ variance, uint64_t npix, float* __restrict__ v0) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * kBlock) {
        const float v = variance[i];
        v0[i] = gn[i].w != 0.0f ? (v > 0.0f ? v : 0.0f) : kDvNoSurface;
    }
}

// out may be the caller's input plane: a lane reads nothing of it
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_denoise_var_export(const float* __restrict__ v, uint64_t npix, float* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * kBlock) {
        const float x = v[i];
        out[i] = x > 0.0f ? x : 0.0f;
    }
}

// sig of a pixel from the nine pre-filter values (kDvNoSurface or any negative: the position does not count; the centre always counts)
TH_D float dv_sigma(const float (&v)[9], float sigma_colour, float var_eps) {
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float g = dv_prefilter_weight(j / 3 - 1) * dv_prefilter_weight(j % 3 - 1);
        if (v[j] >= 0.0f) {
            gs += g * v[j];
            gw += g;
        }
    }
    const float gv = gs / gw;
    const float sd = sqrt_(gv);
    return sigma_colour * sd + var_eps;
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_denoise_var_atrous(const float4* __restrict__ gn, const float4* __restrict__ gp, const float4* __restrict__ cin,
                                                                          const float* __restrict__ vin, float4* __restrict__ cout, float* __restrict__ vout, int width, int height,
                                                                          int step, DenoiseWeights sg, float var_eps) {
    const int x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1)), y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 n4 = gn[at], c4 = cin[at];
    if (n4.w == 0.0f) {
        cout[at] = c4;
        vout[at] = kDvNoSurface;
        return;
    }
    const float4 p4 = gp[at];
    float pv[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {  // unit offsets at every step; a position outside the image does not count
        const int qx = x + (j % 3 - 1), qy = y + (j / 3 - 1);
        const bool in = qx >= 0 && qx < width && qy >= 0 && qy < height;
        const float v = vin[in ? (size_t)qy * (size_t)width + (size_t)qx : at];
        pv[j] = in ? v : kDvNoSurface;
    }
    DenoiseWeights sp = sg;
    sp.sigma_colour = dv_sigma(pv, sg.sigma_colour, var_eps);
    const f3 np = mk3(n4.x, n4.y, n4.z), pp = mk3(p4.x, p4.y, p4.z);
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    float ws = 0.0f, vsum = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        const bool in_y = qy >= 0 && qy < height;
        const size_t row = (size_t)(in_y ? qy : y) * (size_t)width;
        float4 nq[5], pq[5], cq[5];
        float vq[5];
        bool ok[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int qx = x + step * (t - 2);
            ok[t] = in_y && qx >= 0 && qx < width;
            const size_t q = row + (size_t)(ok[t] ? qx : x);
            nq[t] = gn[q];
            pq[t] = gp[q];
            cq[t] = cin[q];
            vq[t] = vin[q];
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
            if (ok[t] && nq[t].w != 0.0f) {
                const float w = dn_weight(dn_kernel(dy) * dn_kernel(t - 2), np, pp, c4.w, nq[t], pq[t], cq[t].w, sp);
                sum.x += w * cq[t].x;
                sum.y += w * cq[t].y;
                sum.z += w * cq[t].z;
                ws += w;
                vsum += (w * w) * vq[t];
            }
    }
    const f3 c = sum / ws;
    cout[at] = make_float4(c.x, c.y, c.z, to_Y(c));
    const float vn = vsum / (ws * ws);
    vout[at] = vn > 0.0f ? vn : 0.0f;
}

// LDS-staged variant for step S: k_denoise_atrous_lds's tile with the variance beside it, (16 + 4 S)^2 pixels of 52 bytes (S = 1: 20.3 KB, 2: 29.3 KB).  Pixels outside the
// image are staged with a zero surface flag and the sentinel.  The halo of 2 S >= 2 covers the pre-filter's unit offsets.
template <int S>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_denoise_var_atrous_lds(const float4* __restrict__ gn, const float4* __restrict__ gp, const float4* __restrict__ cin,
                                                                              const float* __restrict__ vin, float4* __restrict__ cout, float* __restrict__ vout, int width, int height,
                                                                              DenoiseWeights sg, float var_eps) {
    constexpr int TW = kDnTile + 4 * S, NT = TW * TW;
    __shared__ float4 s_n[NT], s_p[NT], s_c[NT];
    __shared__ float s_v[NT];
    const int x0 = (int)blockIdx.x * kDnTile - 2 * S, y0 = (int)blockIdx.y * kDnTile - 2 * S;
    for (int t = (int)threadIdx.x; t < NT; t += kDnTile * kDnTile) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
        float v = kDvNoSurface;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            a = gn[q];
            b = gp[q];
            c = cin[q];
            v = vin[q];
        }
        s_n[t] = a;
        s_p[t] = b;
        s_c[t] = c;
        s_v[t] = v;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const int lc = (ly + 2 * S) * TW + lx + 2 * S;
    const float4 n4 = s_n[lc], c4 = s_c[lc];
    if (n4.w == 0.0f) {
        cout[at] = c4;
        vout[at] = kDvNoSurface;
        return;
    }
    const float4 p4 = s_p[lc];
    float pv[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) pv[j] = s_v[lc + (j / 3 - 1) * TW + (j % 3 - 1)];
    DenoiseWeights sp = sg;
    sp.sigma_colour = dv_sigma(pv, sg.sigma_colour, var_eps);
    const f3 np = mk3(n4.x, n4.y, n4.z), pp = mk3(p4.x, p4.y, p4.z);
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    float ws = 0.0f, vsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int q = lc + (S * dy) * TW + S * dx;
            const float4 nq = s_n[q];
            if (nq.w != 0.0f) {
                const float4 pq = s_p[q], cq = s_c[q];
                const float w = dn_weight(dn_kernel(dy) * dn_kernel(dx), np, pp, c4.w, nq, pq, cq.w, sp);
                sum.x += w * cq.x;
                sum.y += w * cq.y;
                sum.z += w * cq.z;
                ws += w;
                vsum += (w * w) * s_v[q];
            }
        }
    const f3 c = sum / ws;
    cout[at] = make_float4(c.x, c.y, c.z, to_Y(c));
    const float vn = vsum / (ws * ws);
    vout[at] = vn > 0.0f ? vn : 0.0f;
}

}  // namespace th
