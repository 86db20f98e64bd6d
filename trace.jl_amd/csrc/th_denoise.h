// th_denoise.h — edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) on a path / Whitted film, guided by the three planes of trhip_render_aov
// (include/tracehip.h, trhip_denoise; the arithmetic is specified in docs/design/12-denoise.md and every line below is one Float32 operation of that text).
//
//   k_denoise_prepare   film + planes -> per pixel {n, surface flag} {p, 0} {c, Y} {a, 0}: the guides, the (demodulated) linear RGB and its luminance, the clamped base colour
//   k_denoise_atrous    one iteration at step s: 25 taps of three 16-byte loads per surface pixel, straight from memory
//   k_denoise_atrous_lds   steps 1 and 2: the same iteration with the block's pixels and their halo of 2 s staged in LDS first (where a value is read from changes, no sum does)
//   k_denoise_finish    {c, Y} -> the film's XYZ sums again (re-modulated, times the pixel's filter weight); pixels that are no surface pixels keep their input bits
//
// The edge-stopping function is Tukey's biweight, plain arithmetic with compact support: no transcendental function, a neighbour across a hard edge weighs exactly 0.
#pragma once
#include "th_kernels.h"

namespace th {

constexpr int kDnTile = 16;  // a block is 16 x 16 pixels, four waves of 16 x 4

struct DenoiseWeights {
    float sigma_colour, sigma_normal, sigma_plane;  // sigma_colour already scaled by 2^-i
};

TH_D float dn_tukey(float x) {
    if (x < 1.0f) {
        const float t = 1.0f - x * x;
        return t * t;
    }
    return 0.0f;
}
TH_D bool dn_finite(float x) { return fabs_(x) < kInf; }  // false for NaN too
TH_D bool dn_finite3(f3 v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z); }

// Steps 1-6 of Prepare (docs/design/12-denoise.md) for one pixel: B the film pixel, P0..P2 its planes.  Returns the surface flag; n, p, c (and a, with demodulation) are
// meaningful only when it is true.  Shared with the temporal pass (th_temporal.h), which calls it without demodulation.
TH_D bool dn_prepare_pixel(const float4& B, const float4& P0, const float4& P1, const float4& P2, uint32_t demodulate, float albedo_floor, float min_coverage, f3& n, f3& p, f3& c, f3& a) {
    const float W = B.w, A = P0.w, H = P1.w;
    bool surface = W > 0.0f && A > 0.0f && H > 0.0f && H >= min_coverage * A;
    n = mk3(0.0f, 0.0f, 0.0f), p = n, c = n, a = n;
    if (surface) {
        const float iH = 1.0f / H;
        n = mk3(P1.x, P1.y, P1.z) * iH;
        const float len = sqrt_(dot(n, n));
        surface = len > 0.0f;
        n = n / len;
        p = mk3(P2.x, P2.y, P2.z) * iH;
        const float iW = 1.0f / W;
        c = xyz_to_rgb(mk3(B.x, B.y, B.z) * iW);
        if (demodulate) {
            const float iA = 1.0f / A;
            a = mk3(P0.x, P0.y, P0.z) * iA;
            a.x = a.x > albedo_floor ? a.x : albedo_floor;
            a.y = a.y > albedo_floor ? a.y : albedo_floor;
            a.z = a.z > albedo_floor ? a.z : albedo_floor;
            c = c / a;
        }
        surface = surface && dn_finite3(n) && dn_finite3(p) && dn_finite3(c);
    }
    return surface;
}

// One pixel per lane, pixels in film order.  planes: [pixel][3] float4 as trhip_render_aov writes them.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(const float4* __restrict__ beauty, const float4* __restrict__ planes, uint64_t npix, uint32_t demodulate, float albedo_floor,
                                                            float min_coverage, float4* __restrict__ gn, float4* __restrict__ gp, float4* __restrict__ col, float4* __restrict__ alb) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * kBlock) {
        const float4 B = beauty[i], P0 = planes[3 * i], P1 = planes[3 * i + 1], P2 = planes[3 * i + 2];
        f3 n, p, c, a;
        const bool surface = dn_prepare_pixel(B, P0, P1, P2, demodulate, albedo_floor, min_coverage, n, p, c, a);
        if (!surface) n = p = c = a = mk3(0.0f, 0.0f, 0.0f);  // never read as a neighbour, carried through the iterations, replaced by the input at the end
        gn[i] = make_float4(n.x, n.y, n.z, surface ? 1.0f : 0.0f);
        gp[i] = make_float4(p.x, p.y, p.z, 0.0f);
        col[i] = make_float4(c.x, c.y, c.z, to_Y(c));
        alb[i] = make_float4(a.x, a.y, a.z, 0.0f);
    }
}

// The weight of neighbour q for pixel p times the tap's kernel weight k, in the specified order.
TH_D float dn_weight(float k, f3 np, f3 pp, float Yp, const float4& nq, const float4& pq, float Yq, const DenoiseWeights& sg) {
    const float wn = dn_tukey((1.0f - dot(np, mk3(nq.x, nq.y, nq.z))) / sg.sigma_normal);
    const float wp = dn_tukey(fabs_(dot(np, mk3(pq.x, pq.y, pq.z) - pp)) / sg.sigma_plane);
    const float wc = dn_tukey(fabs_(Yq - Yp) / sg.sigma_colour);
    return ((k * wn) * wp) * wc;
}
TH_D float dn_kernel(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// Plain gather.  Lane (lx, ly) of a 16 x 16 block: a wave is a 16 x 4 patch, so a tap of a wave reads four runs of 256 contiguous bytes per array.  The three loads of a tap are
// issued whether or not the tap counts (at a clamped address), so that the loads of a row of taps are in flight together; what is added is decided afterwards.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_denoise_atrous(const float4* __restrict__ gn, const float4* __restrict__ gp, const float4* __restrict__ cin, float4* __restrict__ cout,
                                                                      int width, int height, int step, DenoiseWeights sg) {
    const int x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1)), y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 n4 = gn[at], c4 = cin[at];
    if (n4.w == 0.0f) {
        cout[at] = c4;
        return;
    }
    const float4 p4 = gp[at];
    const f3 np = mk3(n4.x, n4.y, n4.z), pp = mk3(p4.x, p4.y, p4.z);
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    float ws = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        const bool in_y = qy >= 0 && qy < height;
        const size_t row = (size_t)(in_y ? qy : y) * (size_t)width;
        float4 nq[5], pq[5], cq[5];
        bool ok[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int qx = x + step * (t - 2);
            ok[t] = in_y && qx >= 0 && qx < width;
            const size_t q = row + (size_t)(ok[t] ? qx : x);
            nq[t] = gn[q];
            pq[t] = gp[q];
            cq[t] = cin[q];
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
            if (ok[t] && nq[t].w != 0.0f) {
                const float w = dn_weight(dn_kernel(dy) * dn_kernel(t - 2), np, pp, c4.w, nq[t], pq[t], cq[t].w, sg);
                sum.x += w * cq[t].x;
                sum.y += w * cq[t].y;
                sum.z += w * cq[t].z;
                ws += w;
            }
    }
    const f3 c = sum / ws;
    cout[at] = make_float4(c.x, c.y, c.z, to_Y(c));
}

// LDS-staged variant for step S: the block's 16 x 16 pixels and a halo of 2 S on every side, (16 + 4 S)^2 pixels of 48 bytes (S = 1: 19 KB, 2: 27 KB; at S = 4, 48 KB and three waves per SIMD, it measured slower than the gather: profiles/r9/denoise.txt).  Pixels
// outside the image are staged with a zero surface flag.  The tap loop is the gather's, reading LDS.
template <int S>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_denoise_atrous_lds(const float4* __restrict__ gn, const float4* __restrict__ gp, const float4* __restrict__ cin, float4* __restrict__ cout,
                                                                          int width, int height, DenoiseWeights sg) {
    constexpr int TW = kDnTile + 4 * S, NT = TW * TW;
    __shared__ float4 s_n[NT], s_p[NT], s_c[NT];
    const int x0 = (int)blockIdx.x * kDnTile - 2 * S, y0 = (int)blockIdx.y * kDnTile - 2 * S;
    for (int t = (int)threadIdx.x; t < NT; t += kDnTile * kDnTile) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            a = gn[q];
            b = gp[q];
            c = cin[q];
        }
        s_n[t] = a;
        s_p[t] = b;
        s_c[t] = c;
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
        return;
    }
    const float4 p4 = s_p[lc];
    const f3 np = mk3(n4.x, n4.y, n4.z), pp = mk3(p4.x, p4.y, p4.z);
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    float ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int q = lc + (S * dy) * TW + S * dx;
            const float4 nq = s_n[q];
            if (nq.w != 0.0f) {
                const float4 pq = s_p[q], cq = s_c[q];
                const float w = dn_weight(dn_kernel(dy) * dn_kernel(dx), np, pp, c4.w, nq, pq, cq.w, sg);
                sum.x += w * cq.x;
                sum.y += w * cq.y;
                sum.z += w * cq.z;
                ws += w;
            }
        }
    const f3 c = sum / ws;
    cout[at] = make_float4(c.x, c.y, c.z, to_Y(c));
}

// out may be the beauty buffer itself: a lane reads its pixel before it writes it and touches no other.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_denoise_finish(const float4* beauty, const float4* __restrict__ gn, const float4* __restrict__ col, const float4* __restrict__ alb, uint64_t npix,
                                                           uint32_t demodulate, float4* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * kBlock) {
        float4 B = beauty[i];
        if (gn[i].w != 0.0f) {
            const float4 c4 = col[i];
            f3 c = mk3(c4.x, c4.y, c4.z);
            if (demodulate) {
                const float4 a4 = alb[i];
                c = c * mk3(a4.x, a4.y, a4.z);
            }
            const f3 xyz = rgb_to_xyz(c) * B.w;
            B = make_float4(xyz.x, xyz.y, xyz.z, B.w);
        }
        out[i] = B;
    }
}

}  // namespace th
