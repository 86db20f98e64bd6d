// th_temporal_clip.h — temporal reprojection with variance clipping of the history (Salvi 2016, "An excursion in temporal supersampling"): the reprojected history colour is
// confined, before the blend, to mean +- gamma * sd of the NEW frame's colours in a (2 R + 1)^2 window around the pixel (include/tracehip.h, trhip_temporal_clip; the arithmetic
// is specified in docs/design/15-temporal-clip.md; the steps and the LDS layout are in th_temporal_steps.h).
//
//   k_temporal_clip<R>   film + planes + previous history -> film + history.  A block is 16 x 16 pixels, a wave a 16 x 4 patch (k_temporal<true>'s mapping).  Stage the
//                        window, fetch the centre from LDS, window statistics, gather, clip, blend, write.  The window reads neighbours' film pixels, so `out` must NOT be the
//                        film (the host side sees to that).
#pragma once
#include "th_temporal.h"

namespace th {

template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_clip(const float4* __restrict__ beauty, const float4* __restrict__ planes, const float4* __restrict__ history, int width,
                                                                     int height, TemporalConst k, float gamma, float4* __restrict__ out, float4* __restrict__ out_history) {
    constexpr int TW = kDnTile + 2 * R;
    __shared__ float4 s_nf[TW * kTcStride4], s_pc[TW * kTcStride4];
    __shared__ float2 s_c[TW * kTcStride2];
    tc_stage_window<R>(beauty, planes, width, height, k.min_coverage, s_nf, s_pc, s_c);
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at];
    const int l4 = (ly + R) * kTcStride4 + lx + R, l2 = (ly + R) * kTcStride2 + lx + R;
    const float4 n4 = s_nf[l4];
    if (n4.w == 0.0f) {
        tp_write_no_surface(at, B, out, out_history);
        return;
    }
    const float4 p4 = s_pc[l4];
    const float2 c2 = s_c[l2];
    const f3 n = mk3(n4.x, n4.y, n4.z), p = mk3(p4.x, p4.y, p4.z), c = mk3(p4.w, c2.x, c2.y);
    f3 lo, hi;
    tc_window_stats<R>(s_nf, s_pc, s_c, l4, l2, n, p, k, gamma, lo, hi);
    f3 cn = c, ch;
    float Nn = 1.0f, Nh;
    TpTapNothing tap;
    if (tp_gather(history, true, k, p, n, width, height, at, tap, ch, Nh)) {
        tc_clip(ch, lo, hi);
        tp_blend(c, ch, Nh, 1.0f, k.max_history, cn, Nn);
    }
    tp_write_history(at, cn, Nn, n, p, B.w, out, out_history);
}

}  // namespace th
