// th_temporal.h — temporal reprojection of a path film (SVGF's first step, Schied et al. 2017, section 4.1): the previous frame's accumulated colour is fetched through the
// previous camera, validated against the feature planes and blended with the new frame (include/tracehip.h, trhip_temporal; the arithmetic is specified in
// docs/design/14-temporal.md; the steps are in th_temporal_steps.h).
//
//   k_temporal<PATCH>   film + planes + previous history -> film + history: fetch, prepare, gather, blend, write.  One pixel per lane: 64 B streamed in, four gathered 48-byte history records, 64 B out.  No LDS.
//                       PATCH = false: lanes in film order (a wave is 64 consecutive pixels of a row); PATCH = true: the à-trous kernel's blocks of 16 x 16, a wave a 16 x 4 patch.
//                       The mapping decides which lane computes a pixel, never what it computes.
#pragma once
#include "th_temporal_steps.h"

namespace th {

// history: [pixel][3] float4 {c, N} {n, surface flag} {p, 0} of the previous frame, or nullptr.  out may be the beauty buffer itself: a lane reads its pixel before it writes it and
// touches no other; out_history overlaps nothing that is read (checked by the host side).
template <bool PATCH>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal(const float4* beauty, const float4* __restrict__ planes, const float4* __restrict__ history, int width, int height,
                                                                TemporalConst k, float4* out, float4* __restrict__ out_history) {
    int x, y;
    if (PATCH) {
        x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1));
        y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
        if (x >= width || y >= height) return;
    } else {
        const uint64_t i = (uint64_t)blockIdx.x * (kDnTile * kDnTile) + threadIdx.x;
        if (i >= (uint64_t)width * (uint64_t)height) return;
        y = (int)(i / (uint64_t)width);
        x = (int)(i - (uint64_t)y * (uint64_t)width);
    }
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at], P0 = planes[3 * at], P1 = planes[3 * at + 1], P2 = planes[3 * at + 2];
    f3 n, p, c, unused;
    if (!dn_prepare_pixel(B, P0, P1, P2, 0u, 0.0f, k.min_coverage, n, p, c, unused)) {
        tp_write_no_surface(at, B, out, out_history);
        return;
    }
    f3 cn = c, ch;
    float Nn = 1.0f, Nh;
    TpTapNothing tap;
    if (tp_gather(history, true, k, p, n, width, height, at, tap, ch, Nh)) tp_blend(c, ch, Nh, 1.0f, k.max_history, cn, Nn);
    tp_write_history(at, cn, Nn, n, p, B.w, out, out_history);
}

}  // namespace th
