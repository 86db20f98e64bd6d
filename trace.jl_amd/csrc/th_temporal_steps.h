// th_temporal_steps.h — the steps of the temporal preview kernels, one copy of each.  k_temporal, k_temporal_motion, k_temporal_split, k_temporal_clip, k_temporal_clip_motion,
// k_temporal_moments, k_temporal_upsample and k_temporal_upsample_motion are sequences of these; a pass that is "a parent plus one step" is written as another sequence, not as
// another copy.  Every line is one Float32 operation of the design texts (docs/design/14-temporal.md, 15-temporal-clip.md, 20-motion.md), in their order; the build has
// -ffp-contract=off -fno-fast-math, so a line computes the same bits here as it did inside a kernel.
//
//   tp_carry             step 1b: the pixel's surface carried back to where its rigid body was in the previous frame
//   tp_gather            steps 2-3: projection through the previous camera, the four history taps, their acceptance test and weighted sums
//   tp_blend             step 4: the new colour blended into the history's, with the non-finite restart
//   tp_write_history     the epilogue of a surface pixel
//   tp_write_no_surface  the epilogue of a pixel that keeps no history
//   tc_stage_window, tc_window_stats, tc_clip   the new frame's window of k_temporal_clip<R> and k_temporal_clip_motion<R>, and the clip to it
//   tc_counts            which pixels of a window count: those two kernels' walk and k_temporal_moments'
#pragma once
#include "th_denoise.h"

namespace th {

struct TemporalConst {
    float m[12];  // the previous frame's world-to-pixel matrix, row-major 3 x 4 (trhip_sensor_world_to_pixel)
    float max_history, sigma_normal, sigma_plane, min_coverage;
};

constexpr float kTpMaxPosition = 1048576.0f;  // 2^20: a reprojected position at or beyond it (or not finite) has no history

// A pixel that keeps no history: `value` goes to the film, three zero records to the history.
TH_D void tp_write_no_surface(size_t at, const float4& value, float4* out, float4* out_history) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[at] = value;
    out_history[3 * at] = zero;
    out_history[3 * at + 1] = zero;
    out_history[3 * at + 2] = zero;
}

// A surface pixel: the film gets cn at weight w, the history {cn, Nn} and the CURRENT surface (under motion: the next frame's previous world).
TH_D void tp_write_history(size_t at, const f3& cn, float Nn, const f3& n, const f3& p, float w, float4* out, float4* out_history) {
    const f3 xyz = rgb_to_xyz(cn) * w;
    out[at] = make_float4(xyz.x, xyz.y, xyz.z, w);
    out_history[3 * at] = make_float4(cn.x, cn.y, cn.z, Nn);
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
}

// pr, nr: the pixel's surface in the previous frame's world; a static pixel keeps its bits.  False when the carried surface is not finite.  prim, body_of_prim (n_prims words
// or nullptr) and bodies (n_bodies x 12 floats or nullptr, read as floats: 4-byte aligned is enough) are caller data of ANY bit content: every index is compared with its
// array's size before it becomes an address.  The caller loads prim: where that load sits is measured per kernel.
TH_D bool tp_carry(int prim, const uint32_t* __restrict__ body_of_prim, const float* __restrict__ bodies, uint32_t n_prims, uint32_t n_bodies, const f3& p, const f3& n, f3& pr,
                   f3& nr) {
    pr = p;
    nr = n;
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
    return carried;
}

// What a history tap carries beside its three records: nothing, for every kernel but k_temporal_moments (TmTapMoments, th_temporal_moments.h).  load(t, q) is called in the
// batch of the history loads, add(t, b) for an accepted tap of bilinear weight b, finish(sb) once with the sum of the accepted weights.
struct TpTapNothing {
    TH_D void load(int, size_t) {}
    TH_D void add(int, float) {}
    TH_D void finish(float) {}
};

// history: [pixel][3] float4 {c, N} {n, surface flag} {p, 0} of the previous frame, or nullptr.  pr, nr: the surface to look up (tp_carry's, or the pixel's own p, n with
// usable = true).  True when a tap was accepted; ch and Nh are then the history's colour and length there.
template <class Tap>
TH_D bool tp_gather(const float4* __restrict__ history, bool usable, const TemporalConst& k, const f3& pr, const f3& nr, int width, int height, size_t at, Tap& tap, f3& ch, float& Nh) {
    bool found = false;
    const float hx = ((k.m[0] * pr.x + k.m[1] * pr.y) + k.m[2] * pr.z) + k.m[3];
    const float hy = ((k.m[4] * pr.x + k.m[5] * pr.y) + k.m[6] * pr.z) + k.m[7];
    const float hz = ((k.m[8] * pr.x + k.m[9] * pr.y) + k.m[10] * pr.z) + k.m[11];
    if (history && usable) {
        // hz > 0 is tested beside the position, not around the division: one divergent region less.  k_temporal_upsample_motion sits at the SGPR limit and spills two with the
        // tests nested; a lane behind the camera divides for nothing and is refused all the same
        const float fx = hx / hz, fy = hy / hz;
        if (hz > 0.0f && fabs_(fx) < kTpMaxPosition && fabs_(fy) < kTpMaxPosition) {  // false for NaN too
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float tx = fx - x0, ty = fy - y0;
            const int ix = (int)x0, iy = (int)y0;
            // the loads of the four taps are issued whether or not a tap counts (at a clamped address), so that they are in flight together
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
                tap.load(t, q);
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
                    tap.add(t, b);
                }
            }
            if (sb > 0.0f) {
                found = true;
                ch = sc / sb;
                Nh = sN / sb;
                tap.finish(sb);
            }
        }
    }
    return found;
}

// The new colour c, observed with confidence kappa, blended into the history's ch of length Nh.  kappa = 1.0f is the count-weighted blend (1 / Nn, restart at 1); the
// upsampling kernels pass the confidence of their guided taps.  False when the blend was not finite and the pixel restarted from c.
TH_D bool tp_blend(const f3& c, const f3& ch, float Nh, float kappa, float max_history, f3& cn, float& Nn) {
    const float N1 = Nh + kappa;
    Nn = N1 < max_history ? N1 : max_history;
    const float a = kappa / Nn;
    cn = ch + a * (c - ch);
    const bool kept = dn_finite3(cn);
    if (!kept) {
        cn = c;
        Nn = kappa;
    }
    return kept;
}

// The window of the new frame around each pixel of a 16 x 16 block, staged in LDS as {n, flag} {p, c.x} {c.y, c.z}, 40 bytes per pixel.  A wave's 16-byte read is served in
// four groups of 16 lanes, each made of eight lanes of one row of the patch and eight of the next that between them cover the 16 column residues once, over 64 banks of 4
// bytes: the 16 lanes hit 64 different banks iff the row stride is a multiple of 16 records.  Its 8-byte read is served in two groups of 32 lanes (two rows of the patch):
// conflict-free iff the stride is 16 mod 32 records.  The rows are 18 to 22 records long, hence strides of 32 records for the two float4 arrays and 48 for the float2 array:
// 1408 bytes per row, 30976 bytes at R = 3 (five blocks per CU), 28160 at R = 2, 25344 at R = 1.
constexpr int kTcStride4 = 32;  // records per staged row of the float4 arrays
constexpr int kTcStride2 = 48;  // ... of the float2 array

// The block runs dn_prepare_pixel for its (16 + 2 R)^2 pixels; positions outside the image are staged as non-surface.  The caller's __syncthreads() follows.
template <int R>
TH_D void tc_stage_window(const float4* __restrict__ beauty, const float4* __restrict__ planes, int width, int height, float min_coverage, float4* s_nf, float4* s_pc, float2* s_c) {
    constexpr int TW = kDnTile + 2 * R, NT = TW * TW;
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
            if (dn_prepare_pixel(Bq, Q0, Q1, Q2, 0u, 0.0f, min_coverage, nq, pq, cq, unused)) {
                a = make_float4(nq.x, nq.y, nq.z, 1.0f);
                b = make_float4(pq.x, pq.y, pq.z, cq.x);
                d = make_float2(cq.y, cq.z);
            }
        }
        s_nf[ty * kTcStride4 + tx] = a;
        s_pc[ty * kTcStride4 + tx] = b;
        s_c[ty * kTcStride2 + tx] = d;
    }
}

// Whether a staged neighbour {nq: n, flag} {pq: p, .} counts in the window of the pixel with surface n, p: when it is a surface pixel on the centre's surface.  The centre
// itself counts unconditionally: the walks say so.
TH_D bool tc_counts(const float4& nq, const float4& pq, const f3& n, const f3& p, const TemporalConst& k) {
    return nq.w != 0.0f && 1.0f - dot(n, mk3(nq.x, nq.y, nq.z)) < k.sigma_normal && fabs_(dot(n, mk3(pq.x, pq.y, pq.z) - p)) < k.sigma_plane;
}

// lo, hi = mean -+ gamma * sd of the new frame's colours over the (2 R + 1)^2 window of the pixel staged at l4 (float4 arrays) and l2 (float2 array), with the CURRENT n, p (the
// window is this frame's: no motion enters it).  Walked from LDS dy outer and dx inner, summing in that order: no tree, no reordering.
template <int R>
TH_D void tc_window_stats(const float4* s_nf, const float4* s_pc, const float2* s_c, int l4, int l2, const f3& n, const f3& p, const TemporalConst& k, float gamma, f3& lo, f3& hi) {
    f3 m1 = mk3(0.0f, 0.0f, 0.0f), m2 = m1;
    float cnt = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int q4 = l4 + dy * kTcStride4 + dx, q2 = l2 + dy * kTcStride2 + dx;
            const float4 nq = s_nf[q4], pq = s_pc[q4];
            const float2 cq = s_c[q2];
            if ((dy == 0 && dx == 0) || tc_counts(nq, pq, n, p, k)) {
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
    lo = mean - gamma * sd;
    hi = mean + gamma * sd;
}

// The history colour confined to [lo, hi]; true when a component moved.  Comparisons with NaN are false, so gamma = +Inf leaves ch as it is and a NaN ch is never "clipped".
TH_D bool tc_clip(f3& ch, const f3& lo, const f3& hi) {
    const bool bx = ch.x < lo.x, ax = ch.x > hi.x, by = ch.y < lo.y, ay = ch.y > hi.y, bz = ch.z < lo.z, az = ch.z > hi.z;
    ch.x = bx ? lo.x : (ax ? hi.x : ch.x);
    ch.y = by ? lo.y : (ay ? hi.y : ch.y);
    ch.z = bz ? lo.z : (az ? hi.z : ch.z);
    return bx || ax || by || ay || bz || az;
}

}  // namespace th
