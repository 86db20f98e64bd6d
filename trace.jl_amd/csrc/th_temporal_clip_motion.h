// th_temporal_clip_motion.h — temporal reprojection with variance clipping of the history for a scene that holds moving rigid bodies (include/tracehip.h,
// trhip_temporal_clip_motion; the arithmetic is specified in docs/design/21-clip-motion.md and every line below is one Float32 operation of that text): k_temporal_clip's window
// statistics of the NEW frame (th_temporal_clip.h), k_temporal_motion's body carry before the history is looked up (th_temporal_motion.h), and one thing neither has: a pixel
// whose history colour was clipped has its history length cut to clip_max_history before the blend, so that a surface a shadow has just left converges at the new frame's rate.
//
//   k_temporal_clip_motion<R>   film + planes + ids + body table + body matrices + previous history -> film + history.  k_temporal_clip<R>'s block of 16 x 16 (a wave a 16 x 4
//                               patch), its LDS staging of {n, flag} {p, c.x} {c.y, c.z} with the strides of 32 and 48 records and its unrolled window walk, unchanged; then the
//                               lane's id word, table word and twelve matrix words, loaded AFTER the walk (loading them before the staging loop measured 0.0829 ms against 0.0817 at R = 3 and
//                               the same registers: docs/design/21-clip-motion.md), the carry, and
//                               the four-tap gather of k_temporal_motion.  The window reads neighbours' film pixels, so `out` must NOT be the film (the host side sees to that).
//
// ids, body_of_prim and bodies are caller data of ANY bit content: every index is compared with its array's size before it becomes an address, and nothing else of them is read.
// ids may be nullptr: every pixel is then static before anything is read.
#pragma once
#include "th_temporal_clip.h"

namespace th {

template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_clip_motion(const float4* __restrict__ beauty, const float4* __restrict__ planes, const float4* __restrict__ history,
                                                                            const int4* __restrict__ ids, const uint32_t* __restrict__ body_of_prim, const float* __restrict__ bodies, int width,
                                                                            int height, TemporalConst k, float gamma, float clip_max_history, uint32_t n_prims, uint32_t n_bodies,
                                                                            float4* __restrict__ out, float4* __restrict__ out_history) {
    constexpr int TW = kDnTile + 2 * R, NT = TW * TW;
    __shared__ float4 s_nf[TW * kTcStride4], s_pc[TW * kTcStride4];
    __shared__ float2 s_c[TW * kTcStride2];
    const int x0 = (int)blockIdx.x * kDnTile - R, y0 = (int)blockIdx.y * kDnTile - R;
    for (int t = (int)threadIdx.x; t < NT; t += kDnTile * kDnTile) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        float2 d = make_float2(0.0f, 0.0f);
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            const float4 Bq = beauty[q], Q0 = planes[3 * q], Q1 = planes[3 * q + 1], Q2 = planes[3 * q + 2];
            f3 nq, pq, cq, unused;
            if (dn_prepare_pixel(Bq, Q0, Q1, Q2, 0u, 0.0f, k.min_coverage, nq, pq, cq, unused)) {
                a = make_float4(nq.x, nq.y, nq.z, 1.0f);
                b = make_float4(pq.x, pq.y, pq.z, cq.x);
                d = make_float2(cq.y, cq.z);
            }
        }
        s_nf[ty * kTcStride4 + tx] = a;
        s_pc[ty * kTcStride4 + tx] = b;
        s_c[ty * kTcStride2 + tx] = d;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at];
    const int l4 = (ly + R) * kTcStride4 + lx + R, l2 = (ly + R) * kTcStride2 + lx + R;
    const float4 n4 = s_nf[l4];
    if (n4.w == 0.0f) {  // no surface pixel: its id is not looked at
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[at] = B;
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        return;
    }
    const float4 p4 = s_pc[l4];
    const float2 c2 = s_c[l2];
    const f3 n = mk3(n4.x, n4.y, n4.z), p = mk3(p4.x, p4.y, p4.z), c = mk3(p4.w, c2.x, c2.y);
    // window statistics of the new frame, with the CURRENT n, p, c (the window is this frame's: no motion enters it): the centre counts unconditionally, a neighbour when it is
    // a surface pixel on the centre's surface
    f3 m1 = mk3(0.0f, 0.0f, 0.0f), m2 = m1;
    float cnt = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int q4 = l4 + dy * kTcStride4 + dx, q2 = l2 + dy * kTcStride2 + dx;
            const float4 nq = s_nf[q4], pq = s_pc[q4];
            const float2 cq = s_c[q2];
            const bool counts = (dy == 0 && dx == 0) || (nq.w != 0.0f && 1.0f - dot(n, mk3(nq.x, nq.y, nq.z)) < k.sigma_normal && fabs_(dot(n, mk3(pq.x, pq.y, pq.z) - p)) < k.sigma_plane);
            if (counts) {
                m1.x += pq.w;
                m1.y += cq.x;
                m1.z += cq.y;
                m2.x += pq.w * pq.w;
                m2.y += cq.x * cq.x;
                m2.z += cq.y * cq.y;
                cnt += 1.0f;
            }
        }
    const f3 mean = m1 / cnt;
    f3 var = m2 / cnt - mean * mean;
    var.x = var.x > 0.0f ? var.x : 0.0f;
    var.y = var.y > 0.0f ? var.y : 0.0f;
    var.z = var.z > 0.0f ? var.z : 0.0f;
    const f3 sd = mk3(sqrt_(var.x), sqrt_(var.y), sqrt_(var.z));
    const f3 lo = mean - gamma * sd, hi = mean + gamma * sd;

    // step 1b: the body.  pr, nr: the pixel's surface in the previous frame's world; a static pixel keeps its bits.  Each test before the next one's memory is touched
    f3 pr = p, nr = n;
    bool carried = true;
    if (ids && body_of_prim && bodies) {
        const int prim = ((const int*)ids)[4 * at];
        if (prim >= 0 && (uint32_t)prim < n_prims) {
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
    }
    f3 cn = c;
    float Nn = 1.0f;
    const float hx = ((k.m[0] * pr.x + k.m[1] * pr.y) + k.m[2] * pr.z) + k.m[3];
    const float hy = ((k.m[4] * pr.x + k.m[5] * pr.y) + k.m[6] * pr.z) + k.m[7];
    const float hz = ((k.m[8] * pr.x + k.m[9] * pr.y) + k.m[10] * pr.z) + k.m[11];
    if (history && carried && hz > 0.0f) {
        const float fx = hx / hz, fy = hy / hz;
        if (fabs_(fx) < kTpMaxPosition && fabs_(fy) < kTpMaxPosition) {  // false for NaN too
            const float fx0 = __builtin_floorf(fx), fy0 = __builtin_floorf(fy);
            const float tx = fx - fx0, ty = fy - fy0;
            const int ix = (int)fx0, iy = (int)fy0;
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
                f3 ch = sc / sb;
                // step 4': comparisons with NaN are false, so gamma = +Inf leaves ch as it is and a NaN ch is never "clipped"
                const bool bx = ch.x < lo.x, ax = ch.x > hi.x, by = ch.y < lo.y, ay = ch.y > hi.y, bz = ch.z < lo.z, az = ch.z > hi.z;
                ch.x = bx ? lo.x : (ax ? hi.x : ch.x);
                ch.y = by ? lo.y : (ay ? hi.y : ch.y);
                ch.z = bz ? lo.z : (az ? hi.z : ch.z);
                const bool clipped = bx || ax || by || ay || bz || az;
                float Nh = sN / sb;
                if (clipped && clip_max_history < Nh) Nh = clip_max_history;
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
