// th_temporal_split.h — the two kernels of a preview that keeps direct and indirect light apart (include/tracehip.h, trhip_temporal_split and trhip_film_add; the arithmetic is
// specified in docs/design/23-direct-split.md and every line below is one Float32 operation of that text).
//
//   k_temporal_split    k_temporal_motion (th_temporal_motion.h) on B' = (B.xyz - D.xyz, B.w): the film's first-hit direct light is taken out before the pixel is prepared, so
//                       that the history holds the indirect remainder alone.  The same 16 x 4 patch per wave, 96 B streamed in (k_temporal_motion's 80 and the direct film's
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
