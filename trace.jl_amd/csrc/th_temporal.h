// th_temporal.h — temporal reprojection of a path film (SVGF's first step, Schied et al. 2017, section 4.1): the previous frame's accumulated colour is fetched through the
// previous camera, validated against the feature planes and blended with the new frame (include/tracehip.h, trhip_temporal; the arithmetic is specified in
// docs/design/14-temporal.md and every line below is one Float32 operation of that text).
//
//   k_temporal<PATCH>   film + planes + previous history -> film + history.  One pixel per lane: 64 B streamed in, four gathered 48-byte history records, 64 B out.  No LDS.
//                       PATCH = false: lanes in film order (a wave is 64 consecutive pixels of a row); PATCH = true: the à-trous kernel's blocks of 16 x 16, a wave a 16 x 4 patch.
//                       The mapping decides which lane computes a pixel, never what it computes.
#pragma once
#include "th_denoise.h"

namespace th {

struct TemporalConst {
    float m[12];  // the previous frame's world-to-pixel matrix, row-major 3 x 4 (trhip_sensor_world_to_pixel)
    float max_history, sigma_normal, sigma_plane, min_coverage;
};

constexpr float kTpMaxPosition = 1048576.0f;  // 2^20: a reprojected position at or beyond it (or not finite) has no history

// history: [pixel][3] float4 {c, N} {n, surface flag} {p, 0} of the previous frame, or nullptr.  out may be the beauty buffer itself: a lane reads its pixel before it writes it and
// touches no other; out_history overlaps nothing that is read (checked by the host side).
template <bool PATCH>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_temporal(const float4* beauty, const float4* __restrict__ planes, const float4* __restrict__ history, int width, int height,
                                                                TemporalConst k, float4* out, float4* __restrict__ out_history) {
    int x, y;
    if (PATCH) {
        x = (int)blockIdx.x * kDnTile + (int)(threadIdx.x & (kDnTile - 1));
        y = (int)blockIdx.y * kDnTile + (int)(threadIdx.x / kDnTile);
        if (x >= width || y >= height) return;
    } else {
        const uint64_t i = (uint64_t)blockIdx.x * (kDnTile * kDnTile) + threadIdx.x;
        if (i >= (uint64_t)width * (uint64_t)height) return;
        y = (int)(i / (uint64_t)width);
        x = (int)(i - (uint64_t)y * (uint64_t)width);
    }
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 B = beauty[at], P0 = planes[3 * at], P1 = planes[3 * at + 1], P2 = planes[3 * at + 2];
    f3 n, p, c, unused;
    if (!dn_prepare_pixel(B, P0, P1, P2, 0u, 0.0f, k.min_coverage, n, p, c, unused)) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[at] = B;
        out_history[3 * at] = zero;
        out_history[3 * at + 1] = zero;
        out_history[3 * at + 2] = zero;
        return;
    }
    f3 cn = c;
    float Nn = 1.0f;
    const float hx = ((k.m[0] * p.x + k.m[1] * p.y) + k.m[2] * p.z) + k.m[3];
    const float hy = ((k.m[4] * p.x + k.m[5] * p.y) + k.m[6] * p.z) + k.m[7];
    const float hz = ((k.m[8] * p.x + k.m[9] * p.y) + k.m[10] * p.z) + k.m[11];
    if (history && hz > 0.0f) {
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
                const bool accepted = inside[t] && h1[t].w == 1.0f && h0[t].w > 0.0f && 1.0f - dot(n, mk3(h1[t].x, h1[t].y, h1[t].z)) < k.sigma_normal &&
                                      fabs_(dot(n, mk3(h2[t].x, h2[t].y, h2[t].z) - p)) < k.sigma_plane;
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
    out_history[3 * at + 1] = make_float4(n.x, n.y, n.z, 1.0f);
    out_history[3 * at + 2] = make_float4(p.x, p.y, p.z, 0.0f);
}

}  // namespace th
