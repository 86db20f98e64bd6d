// th_temporal_moments.h — temporal reprojection that carries the first two moments of the luminance the denoiser compares, and a per-pixel variance estimate (SVGF, Schied et
// al. 2017, section 4.2): k_temporal's colour and history, untouched, with the moments blended along the same taps and a spatial estimate over k_temporal_clip<3>'s window
// where the history is short (include/tracehip.h, trhip_temporal_moments; the arithmetic is specified in docs/design/16-variance.md and every line below, like every line of
// the steps in th_temporal_steps.h, is one Float32 operation of that text).
//
//   k_temporal_moments   film + planes + previous history + previous moments -> film + history + moments + variance.  k_temporal_clip<3>'s frame: a block is
//                        16 x 16 pixels, a wave a 16 x 4 patch, dn_prepare_pixel run once for the block's (16 + 6)^2 pixels.  Staged in LDS: what the walk reads, {n, flag} and
//                        {p, Yd}, 32 bytes per pixel at k_temporal_clip's stride of 32 records (its bank argument: 16-byte reads are conflict-free iff the row stride is a
//                        multiple of 16 records), and the colour of the block's own 256 pixels, which the blend needs and no neighbour reads: 22 x 32 x 32 + 4096 = 26624 bytes.
//                        Another payload than tc_stage_window's, so the staging loop is this kernel's own.
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

// The moments of a history tap, loaded in the batch of its history records (tp_gather), and their weighted means over the accepted taps.
struct TmTapMoments {
    const float2* __restrict__ moments;
    float2 mq[4];
    float s1 = 0.0f, s2 = 0.0f, m1h, m2h;
    TH_D void load(int t, size_t q) { mq[t] = moments[q]; }
    TH_D void add(int t, float b) {
        s1 += b * mq[t].x;
        s2 += b * mq[t].y;
    }
    TH_D void finish(float sb) {
        m1h = s1 / sb;
        m2h = s2 / sb;
    }
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
        tp_write_no_surface(at, B, out, out_history);
        out_moments[at] = make_float2(0.0f, 0.0f);
        out_variance[at] = 0.0f;
        return;
    }
    const float4 p4 = s_py[l4], c4 = s_c[ly * kDnTile + lx];
    const f3 n = mk3(n4.x, n4.y, n4.z), p = mk3(p4.x, p4.y, p4.z), c = mk3(c4.x, c4.y, c4.z);
    const float Yd = p4.w;

    f3 cn = c, ch;
    float Nn = 1.0f, Nh, m1 = Yd, m2 = Yd * Yd, vt = 0.0f;
    bool have_vt = false;
    TmTapMoments tap{moments};
    if (tp_gather(history, true, k, p, n, width, height, at, tap, ch, Nh) && tp_blend(c, ch, Nh, 1.0f, k.max_history, cn, Nn)) {  // a colour that restarts takes the moments with it
        const float a = 1.0f / Nn;  // the blend's weight
        const float b1 = tap.m1h + a * (Yd - tap.m1h);
        const float b2 = tap.m2h + a * (Yd * Yd - tap.m2h);
        if (dn_finite(b1) && dn_finite(b2)) {  // else the moments restart; the colour keeps its history
            m1 = b1;
            m2 = b2;
            const float var = m2 - m1 * m1;
            vt = var > 0.0f ? var : 0.0f;
            have_vt = true;
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
                if ((dy == 0 && dx == 0) || tc_counts(nq, pq, n, p, k)) {
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
    tp_write_history(at, cn, Nn, n, p, B.w, out, out_history);
    out_moments[at] = make_float2(m1, m2);
    out_variance[at] = dn_finite(vn) ? vn : 0.0f;
}

}  // namespace th
