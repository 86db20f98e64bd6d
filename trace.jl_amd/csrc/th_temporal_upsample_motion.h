// th_temporal_upsample_motion.h — temporal upsampling for a scene that holds moving rigid bodies (include/tracehip.h, trhip_temporal_upsample_motion; the arithmetic is
// specified in docs/design/22-upsample-motion.md and every line below is one Float32 operation of that text): k_temporal_upsample<R>'s step U on this frame's low film and
// full-size planes (th_temporal_upsample.h), k_temporal_motion's body carry before the full-size history is looked up (th_temporal_motion.h).
//
//   k_temporal_upsample_motion<R>   low film + low planes + full-size planes + ids + body table + body matrices + previous history -> film + history + mask.
//                                   k_temporal_upsample<R>'s block of 16 x 16 (a wave a 16 x 4 patch), its LDS staging of the low footprint and its guided tap loop,
//                                   operation for operation; then the lane's id word, table word and twelve matrix words, loaded AFTER the tap loop (loading them before
//                                   it measured 0.0426 ms against 0.0394 at R = 1: docs/design/22-upsample-motion.md), the carry, and the four-tap gather with its twelve
//                                   loads issued together at clamped addresses.  A pixel that is no surface pixel returns before its id is looked at.
//                                   R = 1 asks for six waves per SIMD, the parent's: without the request the carry costs 81 VGPRs, one more than six waves allow; with it 80,
//                                   no scratch, no spill, and 0.0394 ms against 0.0398.  R = 2 has its parent's 82 VGPRs and five waves either way.
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
    float bfx = (float)((int)blockIdx.x * kDnTile) * k.ax;
    bfx = bfx + k.bx;
    float bfy = (float)((int)blockIdx.y * kDnTile) * k.ay;
    bfy = bfy + k.by;
    const int ox = (int)__builtin_floorf(bfx) + 1 - R, oy = (int)__builtin_floorf(bfy) + 1 - R;
    const int plane = tw * stride;
    for (int t = (int)threadIdx.x; t < tw * tw; t += kDnTile * kDnTile) {
        const int ty = t / tw, tx = t - ty * tw;
        const int gx = ox + tx, gy = oy + ty;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, r3 = r0;
        if (gx >= 0 && gx < lw && gy >= 0 && gy < lh) {
            const size_t q = (size_t)gy * (size_t)lw + (size_t)gx;
            up_low_record(lo_xyzw[q], lo_planes[3 * q], lo_planes[3 * q + 1], lo_planes[3 * q + 2], k, r0, r1, r2, r3);
        }
        const int at = ty * stride + tx;
        s_rec[at] = r0;
        s_rec[plane + at] = r1;
        s_rec[2 * plane + at] = r2;
        s_rec[3 * plane + at] = r3;
    }
    __syncthreads();
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 P0 = hi_planes[3 * at], P1 = hi_planes[3 * at + 1], P2 = hi_planes[3 * at + 2];
    const float A = P0.w, H = P1.w;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(A > 0.0f)) {  // H1
        out[at] = make_float4(0.0f, 0.0f, 0.0f, A);
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        if (mask) mask[at] = 0;
        return;
    }
    // H2
    bool surface = H > 0.0f && H >= k.min_coverage * A;
    f3 n = mk3(0.0f, 0.0f, 0.0f), p = n;
    if (surface) {
        const float iH = 1.0f / H;
        n = mk3(P1.x, P1.y, P1.z) * iH;
        const float len = sqrt_(dot(n, n));
        surface = len > 0.0f;
        n = n / len;
        p = mk3(P2.x, P2.y, P2.z) * iH;
        surface = surface && dn_finite3(n) && dn_finite3(p);
    }
    // H3
    float fx = (float)x * k.ax;
    fx = fx + k.bx;
    float fy = (float)y * k.ay;
    fy = fy + k.by;
    const float fx0 = __builtin_floorf(fx), fy0 = __builtin_floorf(fy);
    const float tx = fx - fx0, ty = fy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    auto staged_at = [&](int qx, int qy) {
        int cx = qx - ox, cy = qy - oy;
        cx = cx < 0 ? 0 : (cx >= tw ? tw - 1 : cx);
        cy = cy < 0 ? 0 : (cy >= tw ? tw - 1 : cy);
        return cy * stride + cx;
    };
    f3 c = mk3(0.0f, 0.0f, 0.0f);
    uint32_t m = 0;
    float kmax = 0.0f;
    if (surface) {  // H4
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
        float ws = 0.0f;
#pragma unroll
        for (int j = 1 - R; j <= R; ++j) {
            const int qy = y0 + j;
            const bool in_y = qy >= 0 && qy < lh;
            const float dy = tu_dist(j, ty);
            const float ky = 1.0f - dy * k.inv_r;
            const float gy = tu_sharp(dy, kk.rho);
            float4 nq[2 * R], pq[2 * R], cq[2 * R];
            bool ok[2 * R];
#pragma unroll
            for (int t = 0; t < 2 * R; ++t) {
                const int qx = x0 + 1 - R + t;
                ok[t] = in_y && qx >= 0 && qx < lw;
                const int q = staged_at(qx, qy);
                nq[t] = s_rec[q];
                pq[t] = s_rec[plane + q];
                cq[t] = s_rec[2 * plane + q];
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
    if (m == 0) {  // H5
        float4 vq[4], uq[4];
        bool ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
            ok[t] = qx >= 0 && qx < lw && qy >= 0 && qy < lh;
            const int q = staged_at(qx, qy);
            vq[t] = s_rec[plane + q];
            uq[t] = s_rec[3 * plane + q];
        }
        f3 su = mk3(0.0f, 0.0f, 0.0f);
        float sb = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float b = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
            if (ok[t] && vq[t].w != 0.0f) {
                su.x += b * uq[t].x;
                su.y += b * uq[t].y;
                su.z += b * uq[t].z;
                sb += b;
            }
        }
        if (sb > 0.0f) {
            const f3 cu = su / sb;
            if (dn_finite3(cu)) {
                c = cu;
                m = surface ? 3u : 2u;
            }
        }
    }
    if (!surface) {  // exactly trhip_upscale's pixel; no history is kept for it
        const f3 xyz = rgb_to_xyz(c) * A;
        out[at] = make_float4(xyz.x, xyz.y, xyz.z, A);
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        if (mask) mask[at] = (uint8_t)m;
        return;
    }
    // the confidence
    float kappa = 0.0f;
    if (m == 1)
        kappa = kmax > kk.kappa0 ? kmax : kk.kappa0;
    else if (m == 3)
        kappa = kk.kappa0;
    // step 1b: the body.  pr, nr: the pixel's surface in the previous frame's world; a static pixel keeps its bits.  Each test before the next one's memory is touched
    f3 pr = p, nr = n;
    bool carried = true;
    if (ids && body_of_prim && bodies) {
        const int prim = ((const int*)ids)[4 * at];
        if (prim >= 0 && (uint32_t)prim < n_prims) {
            const uint32_t body = body_of_prim[(uint32_t)prim];
            if (body < n_bodies) {
                const float* M = bodies + (size_t)12 * body;
                pr.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
                pr.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
                pr.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
                nr.x = (M[0] * n.x + M[1] * n.y) + M[2] * n.z;
                nr.y = (M[4] * n.x + M[5] * n.y) + M[6] * n.z;
                nr.z = (M[8] * n.x + M[9] * n.y) + M[10] * n.z;
                carried = dn_finite3(pr) && dn_finite3(nr);
            }
        }
    }
    // T: step T of 19-temporal-upsample.md with the carried surface in the projection and in both tap tests
    const TemporalConst& tp = kk.tp;
    f3 cn = c;
    float On = kappa;
    bool found = false;
    const float hx = ((tp.m[0] * pr.x + tp.m[1] * pr.y) + tp.m[2] * pr.z) + tp.m[3];
    const float hy = ((tp.m[4] * pr.x + tp.m[5] * pr.y) + tp.m[6] * pr.z) + tp.m[7];
    const float hz = ((tp.m[8] * pr.x + tp.m[9] * pr.y) + tp.m[10] * pr.z) + tp.m[11];
    if (history && carried && hz > 0.0f) {
        const float px = hx / hz, py = hy / hz;
        if (fabs_(px) < kTpMaxPosition && fabs_(py) < kTpMaxPosition) {  // false for NaN too
            const float hx0 = __builtin_floorf(px), hy0 = __builtin_floorf(py);
            const float sx = px - hx0, sy = py - hy0;
            const int ix = (int)hx0, iy = (int)hy0;
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
            float sO = 0.0f, sb = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float b = ((t & 1) ? sx : 1.0f - sx) * ((t >> 1) ? sy : 1.0f - sy);
                const bool accepted = inside[t] && h1[t].w == 1.0f && h0[t].w > 0.0f && 1.0f - dot(nr, mk3(h1[t].x, h1[t].y, h1[t].z)) < tp.sigma_normal &&
                                      fabs_(dot(nr, mk3(h2[t].x, h2[t].y, h2[t].z) - pr)) < tp.sigma_plane;
                if (accepted) {
                    sc.x += b * h0[t].x;
                    sc.y += b * h0[t].y;
                    sc.z += b * h0[t].z;
                    sO += b * h0[t].w;
                    sb += b;
                }
            }
            if (sb > 0.0f) {
                found = true;
                const f3 ch = sc / sb;
                const float Oh = sO / sb;
                const float O1 = Oh + kappa;
                On = O1 < tp.max_history ? O1 : tp.max_history;
                const float a = kappa / On;
                cn = ch + a * (c - ch);
                if (!dn_finite3(cn)) {
                    cn = c;
                    On = kappa;
                }
            }
        }
    }
    const f3 xyz = rgb_to_xyz(cn) * A;
    out[at] = make_float4(xyz.x, xyz.y, xyz.z, A);
    out_history[3 * at] = make_float4(cn.x, cn.y, cn.z, On);
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);  // the CURRENT surface: the next frame's previous world
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
    if (mask) mask[at] = (uint8_t)(m + (found ? 4u : 0u));
}

}  // namespace th
