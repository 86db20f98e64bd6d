// th_temporal_motion.h — temporal reprojection of a path film whose scene holds moving rigid bodies (include/tracehip.h, trhip_temporal_motion; the arithmetic is specified in
// docs/design/20-motion.md and every line below is one Float32 operation of that text): k_temporal (th_temporal.h) with the pixel's surface carried back to where its body was
// in the previous frame before the history is looked up.
//
//   k_temporal_motion   film + planes + ids + body table + body matrices + previous history -> film + history.  One pixel per lane on the à-trous kernel's blocks of 16 x 16 (a
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
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[at] = B;
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        return;
    }
    // step 1b: the body.  pr, nr: the pixel's surface in the previous frame's world; a static pixel keeps its bits
    f3 pr = p, nr = n;
    bool carried = true;
    if (prim >= 0 && (uint32_t)prim < n_prims && body_of_prim && bodies) {
        const uint32_t body = body_of_prim[(uint32_t)prim];
        if (body < n_bodies) {
            const float* A = bodies + (size_t)12 * body;
            pr.x = ((A[0] * p.x + A[1] * p.y) + A[2] * p.z) + A[3];
            pr.y = ((A[4] * p.x + A[5] * p.y) + A[6] * p.z) + A[7];
            pr.z = ((A[8] * p.x + A[9] * p.y) + A[10] * p.z) + A[11];
            nr.x = (A[0] * n.x + A[1] * n.y) + A[2] * n.z;
            nr.y = (A[4] * n.x + A[5] * n.y) + A[6] * n.z;
            nr.z = (A[8] * n.x + A[9] * n.y) + A[10] * n.z;
            carried = dn_finite3(pr) && dn_finite3(nr);
        }
    }
    f3 cn = c;
    float Nn = 1.0f;
    const float hx = ((k.m[0] * pr.x + k.m[1] * pr.y) + k.m[2] * pr.z) + k.m[3];
    const float hy = ((k.m[4] * pr.x + k.m[5] * pr.y) + k.m[6] * pr.z) + k.m[7];
    const float hz = ((k.m[8] * pr.x + k.m[9] * pr.y) + k.m[10] * pr.z) + k.m[11];
    if (history && carried && hz > 0.0f) {
        const float fx = hx / hz, fy = hy / hz;
        if (fabs_(fx) < kTpMaxPosition && fabs_(fy) < kTpMaxPosition) {  // false for NaN too
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float tx = fx - x0, ty = fy - y0;
            const int ix = (int)x0, iy = (int)y0;
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
                const bool accepted = inside[t] && h1[t].w == 1.0f && h0[t].w > 0.0f && 1.0f - dot(nr, mk3(h1[t].x, h1[t].y, h1[t].z)) < k.sigma_normal &&
                                      fabs_(dot(nr, mk3(h2[t].x, h2[t].y, h2[t].z) - pr)) < k.sigma_plane;
                if (accepted) {
                    sc.x += b * h0[t].x;
                    sc.y += b * h0[t].y;
                    sc.z += b * h0[t].z;
                    sN += b * h0[t].w;
                    sb += b;
                }
            }
            if (sb > 0.0f) {
                const f3 ch = sc / sb;
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
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);  // the CURRENT surface: the next frame's previous world
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
}

}  // namespace th
