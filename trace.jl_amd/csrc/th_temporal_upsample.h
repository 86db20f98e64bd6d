// th_temporal_upsample.h — temporal upsampling (TAAU; Karis 2014, "High-quality temporal supersampling"; AMD FSR 2's accumulation pass): a jittered low-resolution path film is
// upscaled onto the full-size planes as th_upscale.h upscales it, and blended into a FULL-SIZE history fetched through the previous camera as th_temporal.h fetches it, each
// pixel trusting the new frame in proportion to how directly a low sample observed it (include/tracehip.h, trhip_temporal_upsample; the arithmetic is specified in
// docs/design/19-temporal-upsample.md and every line below is one Float32 operation of that text).
//
//   k_temporal_upsample<R>   one full-size pixel per lane, blocks of 16 x 16, a wave a 16 x 4 patch.  The block stages the low records of its footprint in LDS exactly as
//                            k_upscale<R> does (same bound, same stride rule, same idle clamp: th_upscale.h), each lane walks its (2 R)^2 guided taps from LDS — keeping, beside the
//                            sums, the largest confidence any tap gave — and then gathers its four history taps as k_temporal does: the twelve loads issued at clamped
//                            addresses before any is used.  One launch; the upscaled film is neither written nor read back.
// Steps U (H1-H5 of 17-upscale.md with both flags off) repeat k_upscale's operations in k_upscale's order, so that with history == nullptr the film and the mask are its bits.
#pragma once
#include "th_temporal.h"
#include "th_upscale.h"

namespace th {

struct TemporalUpsampleConst {
    UpscaleConst up;   // demodulate = coverage = 0; sigma_normal / sigma_plane are the guide's Tukey widths
    TemporalConst tp;  // the previous FULL-SIZE sensor's matrix; sigma_normal / sigma_plane are the history's strict thresholds
    float kappa0, rho;
};

// the distance inside up_tent
TH_D float tu_dist(int i, float t) { return i <= 0 ? t + (float)(-i) : (float)i - t; }

TH_D float tu_sharp(float d, float rho) {
    const float g = 1.0f - d * rho;
    return g > 0.0f ? g : 0.0f;
}

// history: [pixel][3] float4 {c, Omega} {n, surface flag} {p, 0} of the previous frame at FULL size, or nullptr.  tw and stride describe the staged square (dynamic LDS of
// 4 * tw * stride float4).  No output overlaps anything that is read (checked by the host side).
template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal_upsample(const float4* __restrict__ lo_xyzw, const float4* __restrict__ lo_planes, int lw, int lh,
                                                                         const float4* __restrict__ hi_planes, const float4* __restrict__ history, int width, int height,
                                                                         TemporalUpsampleConst kk, int tw, int stride, float4* __restrict__ out, float4* __restrict__ out_history,
                                                                         uint8_t* __restrict__ mask) {
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
    // T: steps 2-3 of 14-temporal.md on the full-size history, then the weighted blend
    const TemporalConst& tp = kk.tp;
    f3 cn = c;
    float On = kappa;
    bool found = false;
    const float hx = ((tp.m[0] * p.x + tp.m[1] * p.y) + tp.m[2] * p.z) + tp.m[3];
    const float hy = ((tp.m[4] * p.x + tp.m[5] * p.y) + tp.m[6] * p.z) + tp.m[7];
    const float hz = ((tp.m[8] * p.x + tp.m[9] * p.y) + tp.m[10] * p.z) + tp.m[11];
    if (history && hz > 0.0f) {
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
                const bool accepted = inside[t] && h1[t].w == 1.0f && h0[t].w > 0.0f && 1.0f - dot(n, mk3(h1[t].x, h1[t].y, h1[t].z)) < tp.sigma_normal &&
                                      fabs_(dot(n, mk3(h2[t].x, h2[t].y, h2[t].z) - p)) < tp.sigma_plane;
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
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
    if (mask) mask[at] = (uint8_t)(m + (found ? 4u : 0u));
}

}  // namespace th
