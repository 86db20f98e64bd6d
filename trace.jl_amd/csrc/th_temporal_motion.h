// th_temporal_motion.h — temporal reprojection of a path film whose scene holds moving rigid bodies (include/tracehip.h, trhip_temporal_motion; the arithmetic is specified in
// docs/design/20-motion.md; the steps are in th_temporal_steps.h): the pixel's surface is carried back to where its body was in the previous frame before the history is
// looked up.
//
//   k_temporal_motion   film + planes + ids + body table + body matrices + previous history -> film + history: fetch (the id word beside the film record), prepare, carry,
//                       gather, blend, write.  One pixel per lane on the à-trous kernel's blocks of 16 x 16 (a
//                       wave is a 16 x 4 patch: the mapping trhip_temporal ships).  80 B streamed in (k_temporal's 64 and the id record's line), one 4-byte and twelve 4-byte
//                       gathered words for a moving pixel, four gathered 48-byte history records, 64 B out.  No LDS.
//
// ids, body_of_prim and bodies are caller data of ANY bit content: every index is compared with its array's size before it becomes an address, and nothing else of them is read.
#pragma once
#include "th_temporal.h"

namespace th {

// ids: [pixel] {prim, material, t, n_hit}, prim alone is read.  body_of_prim: n_prims words or nullptr.  bodies: n_bodies x 12 floats or nullptr (read as floats: 4-byte aligned
// is enough).  history, out, out_history as in k_temporal.
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_motion(const float4* beauty, const float4* __restrict__ planes, const float4* __restrict__ history,
                                                                      const int4* __restrict__ ids, const uint32_t* __restrict__ body_of_prim, const float* __restrict__ bodies, int width,
                                                                      int height, TemporalConst k, uint32_t n_prims, uint32_t n_bodies, float4* out, float4* __restrict__ out_history) {
    const int x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1));
    const int y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at], P0 = planes[3 * at], P1 = planes[3 * at + 1], P2 = planes[3 * at + 2];
    const int prim = ((const int*)ids)[4 * at];
    f3 n, p, c, unused;
    if (!dn_prepare_pixel(B, P0, P1, P2, 0u, 0.0f, k.min_coverage, n, p, c, unused)) {
        tp_write_no_surface(at, B, out, out_history);
        return;
    }
    f3 pr, nr, cn = c, ch;
    float Nn = 1.0f, Nh;
    const bool carried = tp_carry(prim, body_of_prim, bodies, n_prims, n_bodies, p, n, pr, nr);
    TpTapNothing tap;
    if (tp_gather(history, carried, k, pr, nr, width, height, at, tap, ch, Nh)) tp_blend(c, ch, Nh, 1.0f, k.max_history, cn, Nn);
    tp_write_history(at, cn, Nn, n, p, B.w, out, out_history);
}

}  // namespace th
