// th_temporal_split.h — the two kernels of a preview that keeps direct and indirect light apart (include/tracehip.h, trhip_temporal_split and trhip_film_add; the arithmetic is
// specified in docs/design/23-direct-split.md; the steps are in th_temporal_steps.h).
//
//   k_temporal_split    k_temporal_motion's sequence (th_temporal_motion.h) on B' = (B.xyz - D.xyz, B.w): the film's first-hit direct light is taken out before the pixel is
//                       prepared, so that the history holds the indirect remainder alone.  The same 16 x 4 patch per wave, 96 B streamed in (k_temporal_motion's 80 and the direct film's
//                       16), the same gathers, 64 B out.  No LDS.  D lives for three subtractions: it is loaded beside B and dead before dn_prepare_pixel.
//   k_film_add          out.xyz = a.xyz + b.xyz, out.w = a.w: the direct film goes back onto the filtered remainder.  Grid-stride over float4, 48 B per pixel.
//
// ids, body_of_prim and bodies are caller data of ANY bit content, as in k_temporal_motion: every index is compared with its array's size before it becomes an address.  direct
// is read at the lane's own pixel only.
#pragma once
#include "th_temporal.h"

namespace th {

// direct: [pixel] xyzw or nullptr (.w is not looked at).  ids: nullptr when there is no table (every pixel static).  Everything else as in k_temporal_motion.
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_split(const float4* beauty, const float4* __restrict__ direct, const float4* __restrict__ planes,
                                                                     const float4* __restrict__ history, const int4* __restrict__ ids, const uint32_t* __restrict__ body_of_prim,
                                                                     const float* __restrict__ bodies, int width, int height, TemporalConst k, uint32_t n_prims, uint32_t n_bodies,
                                                                     float4* out, float4* __restrict__ out_history) {
    const int x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1));
    const int y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    float4 B = beauty[at];
    const float4 P0 = planes[3 * at], P1 = planes[3 * at + 1], P2 = planes[3 * at + 2];
    const int prim = ids ? ((const int*)ids)[4 * at] : -1;
    // step 0: the indirect remainder.  Without a direct film B keeps its bits (no subtraction of a zero)
    if (direct) {
        const float4 D = direct[at];
        B.x = B.x - D.x;
        B.y = B.y - D.y;
        B.z = B.z - D.z;
    }
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

constexpr int kFilmAddBlock = 256;

// out may be a: each lane reads its pixel of a and b before it writes it
__global__ __launch_bounds__(kFilmAddBlock) void k_film_add(const float4* a, const float4* __restrict__ b, size_t n, float4* out) {
    const size_t stride = (size_t)gridDim.x * kFilmAddBlock;
    for (size_t i = (size_t)blockIdx.x * kFilmAddBlock + threadIdx.x; i < n; i += stride) {
        const float4 A = a[i], Bv = b[i];
        out[i] = make_float4(A.x + Bv.x, A.y + Bv.y, A.z + Bv.z, A.w);
    }
}

}  // namespace th
