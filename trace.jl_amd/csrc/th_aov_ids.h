// th_aov_ids.h — the id plane of a feature-buffer frame (include/tracehip.h, trhip_render_aov_ids; docs/design/20-motion.md): which primitive a film pixel shows.
//
//   k_aov_ids   records -> one 16-byte trhip_aov_id per film pixel: the nearest of the pixel's OWN spp camera samples.  One pixel per lane, order-free, no atomics, no LDS.
//
// It reads word 0 of the 80-byte records k_aov_resolve wrote ({t, prim, b1, b2}: the hit as the walk returned it) for each of the pixel's samples and the material word of the
// winner alone: 16 B per sample and 4 B per pixel in, 16 B out.  The records are in sample-major slot order, so the lanes of a wave read runs of 80-byte strides; the hit
// queue itself is in k_raygen's physical placement and would need that placement inverted per sample.
#pragma once
#include "th_aov.h"

namespace th {

__global__ __launch_bounds__(kBlock) void k_aov_ids(const DeviceSensor* __restrict__ sep, const float4* __restrict__ rec, uint32_t spp, int4* __restrict__ out) {
    const DeviceSensor& se = *sep;
    const uint64_t npix = (uint64_t)se.film_w * (uint64_t)se.film_h;
    const uint64_t nslot = (uint64_t)se.sb_w * (uint64_t)se.band_rows;  // sample pixels of the frame: one batch, one band
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * kBlock) {
        const int fy = (int)(i / (uint64_t)se.film_w), fx = (int)(i - (uint64_t)fy * (uint64_t)se.film_w);
        // the film pixel's own sample pixel, as k_aov_gather places it: X = crop_min + array index, an integer below 2^24
        const int sx = (int)(se.crop_min[0] + (float)fx), sy = (int)(se.crop_min[1] + (float)fy);
        int best_prim = -1, best_material = -1;
        float best_t = kInf;
        uint32_t n_hit = 0;
        if (sx >= se.sb_min[0] && sx <= se.sb_max[0] && sy >= se.band_y0 && sy < se.band_y0 + se.band_rows) {
            const uint64_t pix = (uint64_t)(sy - se.band_y0) * (uint64_t)se.sb_w + (uint64_t)(sx - se.sb_min[0]);
            uint64_t best_at = 0;
            for (uint32_t s = 0; s < spp; ++s) {
                const uint64_t at = (uint64_t)s * nslot + pix;
                const float4 r0 = rec[(size_t)kAovWords * at];
                const int prim = __float_as_int(r0.y);
                if (prim < 0) continue;
                ++n_hit;
                // the first candidate is any t that is not NaN; afterwards strictly smaller only, so ties stay with the lowest s and a NaN never wins
                if (best_prim < 0 ? r0.x == r0.x : r0.x < best_t) {
                    best_prim = prim;
                    best_t = r0.x;
                    best_at = at;
                }
            }
            if (best_prim >= 0) best_material = __float_as_int(rec[(size_t)kAovWords * best_at + 1].w);
        }
        out[i] = make_int4(best_prim, best_material, __float_as_int(best_t), (int)n_hit);
    }
}

}  // namespace th
