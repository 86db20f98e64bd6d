// th_temporal_moments.h — temporal reprojection that carries the first two moments of the luminance the denoiser compares, and a per-pixel variance estimate (SVGF, Schied et
// al. 2017, section 4.2): k_temporal's pass (th_temporal.h), colour and history untouched, with the moments blended along the same taps and a spatial estimate over
// k_temporal_clip<3>'s window where the history is short (include/tracehip.h, trhip_temporal_moments; the arithmetic is specified in docs/design/16-variance.md and every line
// below is one Float32 operation of that text).
//
//   k_temporal_moments   film + planes + previous history + previous moments -> film + history + moments + variance.  k_temporal_clip<3>'s frame: a block is
//                        16 x 16 pixels, a wave a 16 x 4 patch, dn_prepare_pixel run once for the block's (16 + 6)^2 pixels.  Staged in LDS: what the walk reads, {n, flag} and
//                        {p, Yd}, 32 bytes per pixel at k_temporal_clip's stride of 32 records (its bank argument: 16-byte reads are conflict-free iff the row stride is a
//                        multiple of 16 records), and the colour of the block's own 256 pixels, which the blend needs and no neighbour reads: 22 x 32 x 32 + 4096 = 26624 bytes.
//                        The reprojection comes first and a wave walks its windows only when a lane of it needs the spatial estimate (a ballot).  The form in which
//                        every wave walks, before the reprojection, gave the same bits and measured slower on a steady-state frame (0.078 against 0.0565 ms) and level
//                        on a first frame (profiles/r13/variance.txt); it is not kept.
//                        The staging reads neighbours' film pixels, so `out` must NOT be the film (the host side sees to that).
#pragma once
#include "th_temporal_clip.h"

namespace th {

constexpr int kTmR = 3;  // the window of the spatial estimate: trhip_temporal_clip's at R = 3

struct MomentsConst {
    float albedo_floor, spatial_below;
    uint32_t demodulate;
};

__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_moments(const float4* __restrict__ beauty, const float4* __restrict__ planes, const float4* __restrict__ history,
                                                                        const float2* __restrict__ moments, int width, int height, TemporalConst k, MomentsConst mk,
                                                                        float4* __restrict__ out, float4* __restrict__ out_history, float2* __restrict__ out_moments,
                                                                        float* __restrict__ out_variance) {
    constexpr int R = kTmR, TW = kDnTile + 2 * R, NT = TW * TW;
    __shared__ float4 s_nf[TW * kTcStride4], s_py[TW * kTcStride4], s_c[kDnTile * kDnTile];
    const int x0 = (int)blockIdx.x * kDnTile - R, y0 = (int)blockIdx.y * kDnTile - R;
    for (int t = (int)threadIdx.x; t < NT; t += kDnTile * kDnTile) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, d = a;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            const float4 Bq = beauty[q], Q0 = planes[3 * q], Q1 = planes[3 * q + 1], Q2 = planes[3 * q + 2];
            f3 nq, pq, cq, unused;
            if (dn_prepare_pixel(Bq, Q0, Q1, Q2, 0u, 0.0f, k.min_coverage, nq, pq, cq, unused)) {
                f3 cd = cq;
                if (mk.demodulate) {  // step 5 of the denoiser's Prepare
                    const float iA = 1.0f / Q0.w;
                    f3 al = mk3(Q0.x, Q0.y, Q0.z) * iA;
                    al.x = al.x > mk.albedo_floor ? al.x : mk.albedo_floor;
                    al.y = al.y > mk.albedo_floor ? al.y : mk.albedo_floor;
                    al.z = al.z > mk.albedo_floor ? al.z : mk.albedo_floor;
                    cd = cq / al;
                }
                a = make_float4(nq.x, nq.y, nq.z, 1.0f);
                b = make_float4(pq.x, pq.y, pq.z, to_Y(cd));
                d = make_float4(cq.x, cq.y, cq.z, 0.0f);
            }
        }
        s_nf[ty * kTcStride4 + tx] = a;
        s_py[ty * kTcStride4 + tx] = b;
        if (tx >= R && tx < R + kDnTile && ty >= R && ty < R + kDnTile) s_c[(ty - R) * kDnTile + (tx - R)] = d;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at];
    const int l4 = (ly + R) * kTcStride4 + lx + R;
    const float4 n4 = s_nf[l4];
    if (n4.w == 0.0f) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[at] = B;
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        out_moments[at] = make_float2(0.0f, 0.0f);
        out_variance[at] = 0.0f;
        return;
    }
    const float4 p4 = s_py[l4], c4 = s_c[ly * kDnTile + lx];
    const f3 n = mk3(n4.x, n4.y, n4.z), p = mk3(p4.x, p4.y, p4.z), c = mk3(c4.x, c4.y, c4.z);
    const float Yd = p4.w;

    f3 cn = c;
    float Nn = 1.0f, m1 = Yd, m2 = Yd * Yd, vt = 0.0f;
    bool have_vt = false;
    const float hx = ((k.m[0] * p.x + k.m[1] * p.y) + k.m[2] * p.z) + k.m[3];
    const float hy = ((k.m[4] * p.x + k.m[5] * p.y) + k.m[6] * p.z) + k.m[7];
    const float hz = ((k.m[8] * p.x + k.m[9] * p.y) + k.m[10] * p.z) + k.m[11];
    if (history && hz > 0.0f) {
        const float fx = hx / hz, fy = hy / hz;
        if (fabs_(fx) < kTpMaxPosition && fabs_(fy) < kTpMaxPosition) {  // false for NaN too
            const float fx0 = __builtin_floorf(fx), fy0 = __builtin_floorf(fy);
            const float tx = fx - fx0, ty = fy - fy0;
            const int ix = (int)fx0, iy = (int)fy0;
            // the twelve history loads and the four moment loads of the taps are issued whether or not a tap counts (at a clamped address), so that they are in flight together
            float4 h0[4], h1[4], h2[4];
            float2 mq[4];
            bool inside[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int qx = ix + (t & 1), qy = iy + (t >> 1);
                inside[t] = qx >= 0 && qx < width && qy >= 0 && qy < height;
                const size_t q = inside[t] ? (size_t)qy * (size_t)width + (size_t)qx : at;
                h0[t] = history[3 * q];
                h1[t] = history[3 * q + 1];
                h2[t] = history[3 * q + 2];
                mq[t] = moments[q];
            }
            f3 sc = mk3(0.0f, 0.0f, 0.0f);
            float sN = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f;
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
                    s1 += b * mq[t].x;
                    s2 += b * mq[t].y;
                }
            }
            if (sb > 0.0f) {
                const f3 ch = sc / sb;
                const float Nh = sN / sb;
                const float N1 = Nh + 1.0f;
                Nn = N1 < k.max_history ? N1 : k.max_history;
                const float a = 1.0f / Nn;
                cn = ch + a * (c - ch);
                if (!dn_finite3(cn)) {  // the colour restarts, and the moments with it
                    cn = c;
                    Nn = 1.0f;
                } else {
                    const float m1h = s1 / sb, m2h = s2 / sb;
                    const float b1 = m1h + a * (Yd - m1h);
                    const float b2 = m2h + a * (Yd * Yd - m2h);
                    if (dn_finite(b1) && dn_finite(b2)) {  // else the moments restart; the colour keeps its history
                        m1 = b1;
                        m2 = b2;
                        const float var = m2 - m1 * m1;
                        vt = var > 0.0f ? var : 0.0f;
                        have_vt = true;
                    }
                }
            }
        }
    }
    const bool temporal = have_vt && !(Nn < mk.spatial_below);
    // the spatial estimate: luminance statistics of the new frame over the window; the centre counts unconditionally, a neighbour when it is a surface pixel on the centre's
    // surface.  Wave-uniform: the walk is skipped by a wave none of whose lanes needs it
    float vs = 0.0f;
    if (__ballot(!temporal) != 0ull) {
        float S1 = 0.0f, S2 = 0.0f, cnt = 0.0f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int q4 = l4 + dy * kTcStride4 + dx;
                const float4 nq = s_nf[q4], pq = s_py[q4];
                const bool counts = (dy == 0 && dx == 0) || (nq.w != 0.0f && 1.0f - dot(n, mk3(nq.x, nq.y, nq.z)) < k.sigma_normal && fabs_(dot(n, mk3(pq.x, pq.y, pq.z) - p)) < k.sigma_plane);
                if (counts) {
                    S1 += pq.w;
                    S2 += pq.w * pq.w;
                    cnt += 1.0f;
                }
            }
        const float mean = S1 / cnt;
        const float var = S2 / cnt - mean * mean;
        vs = var > 0.0f ? var : 0.0f;
    }
    const float v = temporal ? vt : vs;
    if (!(dn_finite(m1) && dn_finite(m2))) m1 = m2 = 0.0f;  // a luminance whose square is not finite leaves no moments behind
    const float vn = v / Nn;
    const f3 xyz = rgb_to_xyz(cn) * B.w;
    out[at] = make_float4(xyz.x, xyz.y, xyz.z, B.w);
    out_history[3 * at] = make_float4(cn.x, cn.y, cn.z, Nn);
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
    out_moments[at] = make_float2(m1, m2);
    out_variance[at] = dn_finite(vn) ? vn : 0.0f;
}

}  // namespace th
