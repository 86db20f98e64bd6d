// th_temporal_clip_motion.h — temporal reprojection with variance clipping of the history for a scene that holds moving rigid bodies (include/tracehip.h,
// trhip_temporal_clip_motion; the arithmetic is specified in docs/design/21-clip-motion.md; the steps are in th_temporal_steps.h): k_temporal_clip's window statistics of the
// NEW frame, k_temporal_motion's body carry before the history is looked up, and one thing neither has: a pixel whose history colour was clipped has its history length cut
// to clip_max_history before the blend, so that a surface a shadow has just left converges at the new frame's rate.
//
//   k_temporal_clip_motion<R>   film + planes + ids + body table + body matrices + previous history -> film + history.  Stage the window, fetch the centre from LDS, window
//                               statistics, fetch the id, carry, gather, clip and cut, blend, write.  The lane's id word, and with it the table word and the twelve matrix
//                               words, is loaded AFTER the window walk: loading it before the staging loop measured 0.0829 ms against 0.0817 at R = 3 and the same registers
//                               (docs/design/21-clip-motion.md).  The window reads neighbours' film pixels, so `out` must NOT be the film (the host side sees to that).
//
// ids may be nullptr: every pixel is then static before anything is read.  A pixel that is no surface pixel returns before its id is looked at.
#pragma once
#include "th_temporal_clip.h"

namespace th {

template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_clip_motion(const float4* __restrict__ beauty, const float4* __restrict__ planes, const float4* __restrict__ history,
                                                                            const int4* __restrict__ ids, const uint32_t* __restrict__ body_of_prim, const float* __restrict__ bodies, int width,
                                                                            int height, TemporalConst k, float gamma, float clip_max_history, uint32_t n_prims, uint32_t n_bodies,
                                                                            float4* __restrict__ out, float4* __restrict__ out_history) {
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
    const int prim = ids ? ((const int*)ids)[4 * at] : -1;
    f3 pr, nr, cn = c, ch;
    float Nn = 1.0f, Nh;
    const bool carried = tp_carry(prim, body_of_prim, bodies, n_prims, n_bodies, p, n, pr, nr);
    TpTapNothing tap;
    if (tp_gather(history, carried, k, pr, nr, width, height, at, tap, ch, Nh)) {
        const bool clipped = tc_clip(ch, lo, hi);  // step 4'
        if (clipped && clip_max_history < Nh) Nh = clip_max_history;
        tp_blend(c, ch, Nh, 1.0f, k.max_history, cn, Nn);
    }
    tp_write_history(at, cn, Nn, n, p, B.w, out, out_history);
}

}  // namespace th
