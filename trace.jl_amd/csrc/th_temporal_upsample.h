// th_temporal_upsample.h — temporal upsampling (TAAU; Karis 2014, "High-quality temporal supersampling"; AMD FSR 2's accumulation pass): a jittered low-resolution path film is
// upscaled onto the full-size planes as th_upscale.h upscales it, and blended into a FULL-SIZE history fetched through the previous camera as th_temporal.h fetches it, each
// pixel trusting the new frame in proportion to how directly a low sample observed it (include/tracehip.h, trhip_temporal_upsample; the arithmetic is specified in
// docs/design/19-temporal-upsample.md; the steps are in th_upscale.h, th_temporal_steps.h and below).
//
//   k_temporal_upsample<R>   one full-size pixel per lane, blocks of 16 x 16, a wave a 16 x 4 patch: stage the low footprint (k_upscale<R>'s: same bound, same stride rule, same
//                            idle clamp), surface, guided taps — keeping, beside the sums, the largest confidence any tap gave —, bilinear fallback, confidence, gather, blend,
//                            write.  One launch; the upscaled film is neither written nor read back.
//                            The guided taps H4 stand in this kernel and in k_temporal_upsample_motion<R>, not in a step of their own: as a function they compiled to 86 and
//                            88 VGPRs at R = 2 against 82 and 84 (five waves either way) and measured 0.0544 against 0.0537 ms and 0.0547 against 0.0542
//                            (profiles/r22/temporal_steps.txt); in place both kernels are at their former times.
// Steps U (H1-H5 of 17-upscale.md with both flags off) are k_upscale's operations in k_upscale's order, so that with history == nullptr the film and the mask are its bits.
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

// The confidence with which mask value m observed the pixel: the guided taps' (at least kappa0), kappa0 for the bilinear fallback on a surface pixel, none otherwise.
TH_D float tu_confidence(uint32_t m, float kmax, float kappa0) {
    float kappa = 0.0f;
    if (m == 1)
        kappa = kmax > kappa0 ? kmax : kappa0;
    else if (m == 3)
        kappa = kappa0;
    return kappa;
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
    if (surface) {  // H4, with kmax
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
    // T: steps 2-3 of 14-temporal.md on the full-size history, then the weighted blend
    f3 cn = c, ch;
    float On = kappa, Oh;
    TpTapNothing tap;
    const bool found = tp_gather(history, true, kk.tp, p, n, width, height, at, tap, ch, Oh);
    if (found) tp_blend(c, ch, Oh, kappa, kk.tp.max_history, cn, On);
    tp_write_history(at, cn, On, n, p, A, out, out_history);
    if (mask) mask[at] = (uint8_t)(m + (found ? 4u : 0u));
}

}  // namespace th
