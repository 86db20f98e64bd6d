// th_temporal_upsample_motion.h — temporal upsampling for a scene that holds moving rigid bodies (include/tracehip.h, trhip_temporal_upsample_motion; the arithmetic is
// specified in docs/design/22-upsample-motion.md; the steps are in th_upscale.h, th_temporal_upsample.h and th_temporal_steps.h): k_temporal_upsample<R>'s step U on this
// frame's low film and full-size planes, k_temporal_motion's body carry before the full-size history is looked up.
//
//   k_temporal_upsample_motion<R>   low film + low planes + full-size planes + ids + body table + body matrices + previous history -> film + history + mask.
//                                   k_temporal_upsample<R>'s sequence with the id fetch and the carry in front of the gather.  The lane's id word, and with it the table
//                                   word and the twelve matrix words, is loaded AFTER the tap loop (loading it before it measured 0.0426 ms against 0.0394 at R = 1:
//                                   docs/design/22-upsample-motion.md).  A pixel that is no surface pixel returns before its id is looked at.
//                                   R = 1 asks for six waves per SIMD, k_temporal_upsample<1>'s: without the request the carry costs 81 VGPRs, one more than six waves
//                                   allow; with it 80, no scratch, no spill, and 0.0394 ms against 0.0398.  R = 2 has five waves either way.  The kernel uses every SGPR
//                                   there is (106): see tp_gather's guard before nesting a test around it.
//
// ids, body_of_prim and bodies are caller data of ANY bit content: every index is compared with its array's size before it becomes an address, and nothing else of them is read.
// ids may be nullptr: every pixel is then static before anything is read.
#pragma once
#include "th_temporal_upsample.h"

namespace th {

// history: [pixel][3] float4 as in k_temporal_upsample, or nullptr.  ids: [pixel] int4 {prim, ...} at FULL size.  No output overlaps anything that is read (the host side).
template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) __attribute__((amdgpu_waves_per_eu(R == 1 ? 6 : 5))) void k_temporal_upsample_motion(
    const float4* __restrict__ lo_xyzw, const float4* __restrict__ lo_planes, int lw, int lh, const float4* __restrict__ hi_planes, const float4* __restrict__ history,
    const int4* __restrict__ ids, const uint32_t* __restrict__ body_of_prim, const float* __restrict__ bodies, int width, int height, TemporalUpsampleConst kk, int tw, int stride,
    uint32_t n_prims, uint32_t n_bodies, float4* __restrict__ out, float4* __restrict__ out_history, uint8_t* __restrict__ mask) {
    extern __shared__ float4 s_rec[];
    const UpscaleConst& k = kk.up;
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    const UpStaged st = up_stage_low<R>(lo_xyzw, lo_planes, lw, lh, k, tw, stride, s_rec);
    __syncthreads();
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 P0 = hi_planes[3 * at], P1 = hi_planes[3 * at + 1], P2 = hi_planes[3 * at + 2];
    const float A = P0.w;
    if (!(A > 0.0f)) {  // H1
        tp_write_no_surface(at, make_float4(0.0f, 0.0f, 0.0f, A), out, out_history);
        if (mask) mask[at] = 0;
        return;
    }
    // U: H2-H5 of 17-upscale.md with both flags off
    f3 n, p, c = mk3(0.0f, 0.0f, 0.0f);
    const bool surface = up_surface(P1, P2, A, k.min_coverage, n, p);
    int x0, y0;
    float tx, ty;
    up_low_position(x, y, k, x0, y0, tx, ty);
    uint32_t m = 0;
    float kmax = 0.0f;
    if (surface) {  // H4, with kmax: k_temporal_upsample<R>'s, in place for the reason given there
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
        float ws = 0.0f;
#pragma unroll
        for (int j = 1 - R; j <= R; ++j) {
            const int qy = y0 + j;
            const bool in_y = qy >= 0 && qy < st.lh;
            const float dy = tu_dist(j, ty);
            const float ky = 1.0f - dy * k.inv_r;
            const float gy = tu_sharp(dy, kk.rho);
            float4 nq[2 * R], pq[2 * R], cq[2 * R];
            bool ok[2 * R];
#pragma unroll
            for (int t = 0; t < 2 * R; ++t) {
                const int qx = x0 + 1 - R + t;
                ok[t] = in_y && qx >= 0 && qx < st.lw;
                const int q = up_staged_at(st, qx, qy);
                nq[t] = st.rec[q];
                pq[t] = st.rec[st.plane + q];
                cq[t] = st.rec[2 * st.plane + q];
            }
#pragma unroll
            for (int t = 0; t < 2 * R; ++t)
                if (ok[t] && nq[t].w != 0.0f) {
                    const float dx = tu_dist(1 - R + t, tx);
                    const float kx = 1.0f - dx * k.inv_r;
                    const float kw = ky * kx;
                    const float wn = dn_tukey((1.0f - dot(n, mk3(nq[t].x, nq[t].y, nq[t].z))) / k.sigma_normal);
                    const float wp = dn_tukey(fabs_(dot(n, mk3(pq[t].x, pq[t].y, pq[t].z) - p)) / k.sigma_plane);
                    const float w = (kw * wn) * wp;
                    sum.x += w * cq[t].x;
                    sum.y += w * cq[t].y;
                    sum.z += w * cq[t].z;
                    ws += w;
                    const float gx = tu_sharp(dx, kk.rho);
                    const float g = gy * gx;
                    const float e = (g * wn) * wp;
                    kmax = e > kmax ? e : kmax;
                }
        }
        if (ws > 0.0f) {
            const f3 cg = sum / ws;
            if (dn_finite3(cg)) {
                c = cg;
                m = 1;
            }
        }
    }
    if (m == 0) up_bilinear_fallback(st, x0, y0, tx, ty, surface, c, m);
    if (!surface) {  // exactly trhip_upscale's pixel; no history is kept for it
        const f3 xyz = rgb_to_xyz(c) * A;
        tp_write_no_surface(at, make_float4(xyz.x, xyz.y, xyz.z, A), out, out_history);
        if (mask) mask[at] = (uint8_t)m;
        return;
    }
    const float kappa = tu_confidence(m, kmax, kk.kappa0);
    const int prim = ids ? ((const int*)ids)[4 * at] : -1;
    f3 pr, nr, cn = c, ch;
    float On = kappa, Oh;
    const bool carried = tp_carry(prim, body_of_prim, bodies, n_prims, n_bodies, p, n, pr, nr);
    // T: step T of 19-temporal-upsample.md with the carried surface in the projection and in both tap tests
    TpTapNothing tap;
    const bool found = tp_gather(history, carried, kk.tp, pr, nr, width, height, at, tap, ch, Oh);
    if (found) tp_blend(c, ch, Oh, kappa, kk.tp.max_history, cn, On);
    tp_write_history(at, cn, On, n, p, A, out, out_history);
    if (mask) mask[at] = (uint8_t)(m + (found ? 4u : 0u));
}

}  // namespace th
