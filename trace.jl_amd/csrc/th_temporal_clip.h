// th_temporal_clip.h — temporal reprojection with variance clipping of the history (Salvi 2016, "An excursion in temporal supersampling"): k_temporal's pass (th_temporal.h) with
// the reprojected history colour confined, before the blend, to mean +- gamma * sd of the NEW frame's colours in a (2 R + 1)^2 window around the pixel (include/tracehip.h,
// trhip_temporal_clip; the arithmetic is specified in docs/design/15-temporal-clip.md and every line below is one Float32 operation of that text).
//
//   k_temporal_clip<R>   film + planes + previous history -> film + history.  A block is 16 x 16 pixels, a wave a 16 x 4 patch (k_temporal<true>'s mapping).  The block first runs
//                        dn_prepare_pixel for its (16 + 2 R)^2 pixels and stages {n, flag} {p, c.x} {c.y, c.z} in LDS, 40 bytes per pixel; positions outside the image are staged
//                        as non-surface.  Each lane then walks its window from LDS, dy outer and dx inner, summing in that order — no tree, no reordering —, and the
//                        reprojection follows as in k_temporal.  The window reads neighbours' film pixels, so `out` must NOT be the film (the host side sees to that).
//
// LDS layout.  A wave's 16-byte read is served in four groups of 16 lanes, each made of eight lanes of one row of the patch and eight of the next that between them cover the 16
// column residues once, over 64 banks of 4 bytes: the 16 lanes hit 64 different banks iff the row stride is a multiple of 16 records.  Its 8-byte read is served in two groups of
// 32 lanes (two rows of the patch): conflict-free iff the stride is 16 mod 32 records.  The rows are 18 to 22 records long, hence strides of 32 records for the two float4
// arrays and 48 for the float2 array: 1408 bytes per row, 30976 bytes at R = 3 (five blocks per CU), 28160 at R = 2, 25344 at R = 1.
#pragma once
#include "th_temporal.h"

namespace th {

constexpr int kTcStride4 = 32;  // records per staged row of the float4 arrays
constexpr int kTcStride2 = 48;  // ... of the float2 array

template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_clip(const float4* __restrict__ beauty, const float4* __restrict__ planes, const float4* __restrict__ history, int width,
                                                                     int height, TemporalConst k, float gamma, float4* __restrict__ out, float4* __restrict__ out_history) {
    constexpr int TW = kDnTile + 2 * R, NT = TW * TW;
    __shared__ float4 s_nf[TW * kTcStride4], s_pc[TW * kTcStride4];
    __shared__ float2 s_c[TW * kTcStride2];
    const int x0 = (int)blockIdx.x * kDnTile - R, y0 = (int)blockIdx.y * kDnTile - R;
    for (int t = (int)threadIdx.x; t < NT; t += kDnTile * kDnTile) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        float2 d = make_float2(0.0f, 0.0f);
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            const float4 Bq = beauty[q], Q0 = planes[3 * q], Q1 = planes[3 * q + 1], Q2 = planes[3 * q + 2];
            f3 nq, pq, cq, unused;
            if (dn_prepare_pixel(Bq, Q0, Q1, Q2, 0u, 0.0f, k.min_coverage, nq, pq, cq, unused)) {
                a = make_float4(nq.x, nq.y, nq.z, 1.0f);
                b = make_float4(pq.x, pq.y, pq.z, cq.x);
                d = make_float2(cq.y, cq.z);
            }
        }
        s_nf[ty * kTcStride4 + tx] = a;
        s_pc[ty * kTcStride4 + tx] = b;
        s_c[ty * kTcStride2 + tx] = d;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at];
    const int l4 = (ly + R) * kTcStride4 + lx + R, l2 = (ly + R) * kTcStride2 + lx + R;
    const float4 n4 = s_nf[l4];
    if (n4.w == 0.0f) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[at] = B;
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        return;
    }
    const float4 p4 = s_pc[l4];
    const float2 c2 = s_c[l2];
    const f3 n = mk3(n4.x, n4.y, n4.z), p = mk3(p4.x, p4.y, p4.z), c = mk3(p4.w, c2.x, c2.y);
    // window statistics of the new frame: the centre counts unconditionally, a neighbour when it is a surface pixel on the centre's surface
    f3 m1 = mk3(0.0f, 0.0f, 0.0f), m2 = m1;
    float cnt = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int q4 = l4 + dy * kTcStride4 + dx, q2 = l2 + dy * kTcStride2 + dx;
            const float4 nq = s_nf[q4], pq = s_pc[q4];
            const float2 cq = s_c[q2];
            const bool counts = (dy == 0 && dx == 0) || (nq.w != 0.0f && 1.0f - dot(n, mk3(nq.x, nq.y, nq.z)) < k.sigma_normal && fabs_(dot(n, mk3(pq.x, pq.y, pq.z) - p)) < k.sigma_plane);
            if (counts) {
                m1.x += pq.w;
                m1.y += cq.x;
                m1.z += cq.y;
                m2.x += pq.w * pq.w;
                m2.y += cq.x * cq.x;
                m2.z += cq.y * cq.y;
                cnt += 1.0f;
            }
        }
    const f3 mean = m1 / cnt;
    f3 var = m2 / cnt - mean * mean;
    var.x = var.x > 0.0f ? var.x : 0.0f;
    var.y = var.y > 0.0f ? var.y : 0.0f;
    var.z = var.z > 0.0f ? var.z : 0.0f;
    const f3 sd = mk3(sqrt_(var.x), sqrt_(var.y), sqrt_(var.z));
    const f3 lo = mean - gamma * sd, hi = mean + gamma * sd;

    f3 cn = c;
    float Nn = 1.0f;
    const float hx = ((k.m[0] * p.x + k.m[1] * p.y) + k.m[2] * p.z) + k.m[3];
    const float hy = ((k.m[4] * p.x + k.m[5] * p.y) + k.m[6] * p.z) + k.m[7];
    const float hz = ((k.m[8] * p.x + k.m[9] * p.y) + k.m[10] * p.z) + k.m[11];
    if (history && hz > 0.0f) {
        const float fx = hx / hz, fy = hy / hz;
        if (fabs_(fx) < kTpMaxPosition && fabs_(fy) < kTpMaxPosition) {  // false for NaN too
            const float fx0 = __builtin_floorf(fx), fy0 = __builtin_floorf(fy);
            const float tx = fx - fx0, ty = fy - fy0;
            const int ix = (int)fx0, iy = (int)fy0;
            // the twelve loads of the four taps are issued whether or not a tap counts (at a clamped address), so that they are in flight together
            float4 h0[4], h1[4], h2[4];
            bool inside[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int qx = ix + (t & 1), qy = iy + (t >> 1);
                inside[t] = qx >= 0 && qx < width && qy >= 0 && qy < height;
                const size_t q = inside[t] ? (size_t)qy * (size_t)width + (size_t)qx : at;
                h0[t] = history[3 * q];
                h1[t] = history[3 * q + 1];
                h2[t] = history[3 * q + 2];
            }
            f3 sc = mk3(0.0f, 0.0f, 0.0f);
            float sN = 0.0f, sb = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float b = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
                const bool accepted = inside[t] && h1[t].w == 1.0f && h0[t].w > 0.0f && 1.0f - dot(n, mk3(h1[t].x, h1[t].y, h1[t].z)) < k.sigma_normal &&
                                      fabs_(dot(n, mk3(h2[t].x, h2[t].y, h2[t].z) - p)) < k.sigma_plane;
                if (accepted) {
                    sc.x += b * h0[t].x;
                    sc.y += b * h0[t].y;
                    sc.z += b * h0[t].z;
                    sN += b * h0[t].w;
                    sb += b;
                }
            }
            if (sb > 0.0f) {
                f3 ch = sc / sb;
                ch.x = ch.x < lo.x ? lo.x : (ch.x > hi.x ? hi.x : ch.x);  // comparisons with NaN are false: gamma = +Inf leaves ch as it is
                ch.y = ch.y < lo.y ? lo.y : (ch.y > hi.y ? hi.y : ch.y);
                ch.z = ch.z < lo.z ? lo.z : (ch.z > hi.z ? hi.z : ch.z);
                const float Nh = sN / sb;
                const float N1 = Nh + 1.0f;
                Nn = N1 < k.max_history ? N1 : k.max_history;
                const float a = 1.0f / Nn;
                cn = ch + a * (c - ch);
                if (!dn_finite3(cn)) {
                    cn = c;
                    Nn = 1.0f;
                }
            }
        }
    }
    const f3 xyz = rgb_to_xyz(cn) * B.w;
    out[at] = make_float4(xyz.x, xyz.y, xyz.z, B.w);
    out_history[3 * at] = make_float4(cn.x, cn.y, cn.z, Nn);
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
}

}  // namespace th
