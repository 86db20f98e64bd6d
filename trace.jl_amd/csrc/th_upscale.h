// th_upscale.h — joint bilateral upsampling (Kopf et al. 2007) of a low-resolution path film onto a full-size film, guided by the feature planes of both sizes (include/tracehip.h,
// trhip_upscale; the arithmetic is specified in docs/design/17-upscale.md and every line below is one Float32 operation of that text).
//
//   k_upscale<R>   one full-size pixel per lane, blocks of 16 x 16, a wave a 16 x 4 patch.  The block first runs steps L1-L3 for the low pixels its 16 x 16 full-size pixels can
//                  reach and stages their records {n, s} {p, valid} {c} {u} in LDS; each lane then walks its (2 R)^2 guided taps, j outer and i inner, from LDS.  One launch,
//                  no scratch buffer.
// up_stage_low, up_staged_at, up_surface, up_low_position and up_bilinear_fallback are shared with k_temporal_upsample<R> and k_temporal_upsample_motion<R>
// (th_temporal_upsample.h); the guided taps H4 below are k_upscale's own: theirs keep a confidence beside the sums, these apply the two flags.
// A second form was built and measured: a prepare pass writing the 64-byte records of all low pixels to memory, then the same tap loop gathering them, a row of taps' loads
// issued at clamped addresses before any is used.  Same bits; 1.57 x (R = 1) and 1.77 x (R = 2) the staged form's time at 1024^2 <- 512^2 (profiles/r14/upscale.txt), so it was
// removed before this file's first commit, together with its option and its record buffer: no commit holds it, docs/design/17-upscale.md describes it.
//
// The staged footprint.  Full-size pixel x reads low columns floor(fx) + 1 - R .. floor(fx) + R, fx = x * ax + bx.  Over the 16 columns of a block floor(fx) grows by at most
// ceil(15 ax) + 1 (the + 1: the two roundings of fx, under 0.25 each for |fx| < 2^21, which the host side guarantees), so the block stages T = ceil(15 ax) + 1 + 2 R columns and as
// many rows: 13 at ax = 1/2 with R = 2, 20 at ax = 1.  The four words are four arrays with a row stride of 16 records (T <= 16) or 32, the rule of k_temporal_clip for 16-byte
// reads: 4 * 13 * 16 * 16 = 13312 bytes at the 2 x case (R = 2), 4 * 20 * 32 * 16 = 40960 at ratio 1 (three blocks per CU by LDS).  Positions off the low image are staged as records
// with s = valid = 0, which is what "skipped" means.  A local index is clamped into the staged square: memory safety only, the bound above keeps the clamp idle.
#pragma once
#include "th_denoise.h"

namespace th {

struct UpscaleConst {
    float ax, bx, ay, by;
    float inv_r;  // 1 / R: 1 or 0.5
    uint32_t demodulate, coverage;
    float sigma_normal, sigma_plane, albedo_floor, min_coverage;
};

// Steps L1-L3 for one low pixel.
TH_D void up_low_record(const float4& B, const float4& P0, const float4& P1, const float4& P2, const UpscaleConst& k, float4& r0, float4& r1, float4& r2, float4& r3) {
    f3 n, p, c, a;
    bool s = dn_prepare_pixel(B, P0, P1, P2, k.demodulate, k.albedo_floor, k.min_coverage, n, p, c, a);
    if (k.coverage && s) {
        const float v = P1.w / P0.w;
        c = c / mk3(v, v, v);
        s = dn_finite3(c);
    }
    if (!s) n = p = c = mk3(0.0f, 0.0f, 0.0f);
    bool valid = B.w > 0.0f;
    const float iW = 1.0f / B.w;
    f3 u = xyz_to_rgb(mk3(B.x, B.y, B.z) * iW);
    valid = valid && dn_finite3(u);
    if (!valid) u = mk3(0.0f, 0.0f, 0.0f);
    r0 = make_float4(n.x, n.y, n.z, s ? 1.0f : 0.0f);
    r1 = make_float4(p.x, p.y, p.z, valid ? 1.0f : 0.0f);
    r2 = make_float4(c.x, c.y, c.z, 0.0f);
    r3 = make_float4(u.x, u.y, u.z, 0.0f);
}

TH_D float up_tent(int i, float t, float inv_r) {
    const float d = i <= 0 ? t + (float)(-i) : (float)i - t;
    return 1.0f - d * inv_r;
}

// The staged low footprint of a block: four arrays {n, s} {p, valid} {c} {u} of tw rows at a row stride of `stride` records, staged position (0, 0) being low pixel (ox, oy)
// of the lw x lh low image.
struct UpStaged {
    const float4* rec;
    int ox, oy, tw, stride, plane, lw, lh;
};

// The block runs steps L1-L3 for the tw x tw low pixels its 16 x 16 full-size pixels can reach and stages their records in s_rec (4 * tw * stride float4); positions off the
// low image are staged as zero records.  The caller's __syncthreads() follows.
template <int R>
TH_D UpStaged up_stage_low(const float4* __restrict__ lo_xyzw, const float4* __restrict__ lo_planes, int lw, int lh, const UpscaleConst& k, int tw, int stride, float4* s_rec) {
    // the low pixel of staged position (0, 0): the block's first column and row through step H3's two operations
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
    return UpStaged{s_rec, ox, oy, tw, stride, plane, lw, lh};
}

// where low pixel (qx, qy) is staged (clamped into the square)
TH_D int up_staged_at(const UpStaged& s, int qx, int qy) {
    int cx = qx - s.ox, cy = qy - s.oy;
    cx = cx < 0 ? 0 : (cx >= s.tw ? s.tw - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= s.tw ? s.tw - 1 : cy);
    return cy * s.stride + cx;
}

// H2 without its demodulate and coverage branches: whether the full-size pixel of planes P1, P2 with A = P0.w is a surface pixel, and its n, p.
TH_D bool up_surface(const float4& P1, const float4& P2, float A, float min_coverage, f3& n, f3& p) {
    const float H = P1.w;
    bool surface = H > 0.0f && H >= min_coverage * A;
    n = mk3(0.0f, 0.0f, 0.0f);
    p = n;
    if (surface) {
        const float iH = 1.0f / H;
        n = mk3(P1.x, P1.y, P1.z) * iH;
        const float len = sqrt_(dot(n, n));
        surface = len > 0.0f;
        n = n / len;
        p = mk3(P2.x, P2.y, P2.z) * iH;
        surface = surface && dn_finite3(n) && dn_finite3(p);
    }
    return surface;
}

// H3: where full-size pixel (x, y) falls in the low image: low pixel (x0, y0) and the fractions tx, ty.
TH_D void up_low_position(int x, int y, const UpscaleConst& k, int& x0, int& y0, float& tx, float& ty) {
    float fx = (float)x * k.ax;
    fx = fx + k.bx;
    float fy = (float)y * k.ay;
    fy = fy + k.by;
    const float fx0 = __builtin_floorf(fx), fy0 = __builtin_floorf(fy);
    tx = fx - fx0;
    ty = fy - fy0;
    x0 = (int)fx0;
    y0 = (int)fy0;
}

// H5: the bilinear mean of the four low pixels' unguided colours u, where valid.  Sets c and m (3 on a surface pixel, 2 elsewhere) when it has one.
TH_D void up_bilinear_fallback(const UpStaged& s, int x0, int y0, float tx, float ty, bool surface, f3& c, uint32_t& m) {
    float4 vq[4], uq[4];
    bool ok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
        ok[t] = qx >= 0 && qx < s.lw && qy >= 0 && qy < s.lh;
        const int q = up_staged_at(s, qx, qy);
        vq[t] = s.rec[s.plane + q];
        uq[t] = s.rec[3 * s.plane + q];
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

// tw and stride describe the staged square (dynamic LDS of 4 * tw * stride float4).
template <int R>
__global__ __launch_bounds__(kDnTile* kDnTile) void k_upscale(const float4* __restrict__ lo_xyzw, const float4* __restrict__ lo_planes, int lw, int lh, const float4* __restrict__ hi_planes,
                                                               int width, int height, UpscaleConst k, int tw, int stride, float4* __restrict__ out, uint8_t* __restrict__ mask) {
    extern __shared__ float4 s_rec[];
    const int lx = (int)(threadIdx.x & (kDnTile - 1)), ly = (int)(threadIdx.x / kDnTile);
    const int x = (int)blockIdx.x * kDnTile + lx, y = (int)blockIdx.y * kDnTile + ly;
    const UpStaged st = up_stage_low<R>(lo_xyzw, lo_planes, lw, lh, k, tw, stride, s_rec);
    __syncthreads();
    if (x >= width || y >= height) return;
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    const float4 P0 = hi_planes[3 * at], P1 = hi_planes[3 * at + 1], P2 = hi_planes[3 * at + 2];
    const float A = P0.w;
    if (!(A > 0.0f)) {  // H1
        out[at] = make_float4(0.0f, 0.0f, 0.0f, A);
        if (mask) mask[at] = 0;
        return;
    }
    // H2
    f3 n, p, a = mk3(0.0f, 0.0f, 0.0f);
    float v = 0.0f;
    bool surface = up_surface(P1, P2, A, k.min_coverage, n, p);
    if (surface && k.demodulate) {
        const float iA = 1.0f / A;
        a = mk3(P0.x, P0.y, P0.z) * iA;
        a.x = a.x > k.albedo_floor ? a.x : k.albedo_floor;
        a.y = a.y > k.albedo_floor ? a.y : k.albedo_floor;
        a.z = a.z > k.albedo_floor ? a.z : k.albedo_floor;
        surface = dn_finite3(a);
    }
    if (surface && k.coverage) {
        v = P1.w / A;
        surface = dn_finite(v);
    }
    int x0, y0;
    float tx, ty;
    up_low_position(x, y, k, x0, y0, tx, ty);
    f3 c = mk3(0.0f, 0.0f, 0.0f);
    uint32_t m = 0;
    if (surface) {  // H4
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
        float ws = 0.0f;
#pragma unroll
        for (int j = 1 - R; j <= R; ++j) {
            const int qy = y0 + j;
            const bool in_y = qy >= 0 && qy < st.lh;
            const float ky = up_tent(j, ty, k.inv_r);
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
                    const float kx = up_tent(1 - R + t, tx, k.inv_r);
                    const float kk = ky * kx;
                    const float wn = dn_tukey((1.0f - dot(n, mk3(nq[t].x, nq[t].y, nq[t].z))) / k.sigma_normal);
                    const float wp = dn_tukey(fabs_(dot(n, mk3(pq[t].x, pq[t].y, pq[t].z) - p)) / k.sigma_plane);
                    const float w = (kk * wn) * wp;
                    sum.x += w * cq[t].x;
                    sum.y += w * cq[t].y;
                    sum.z += w * cq[t].z;
                    ws += w;
                }
        }
        if (ws > 0.0f) {
            f3 cg = sum / ws;
            if (k.demodulate) cg = cg * a;
            if (k.coverage) cg = cg * v;
            if (dn_finite3(cg)) {
                c = cg;
                m = 1;
            }
        }
    }
    if (m == 0) up_bilinear_fallback(st, x0, y0, tx, ty, surface, c, m);  // H5
    // H6
    const f3 xyz = rgb_to_xyz(c) * A;
    out[at] = make_float4(xyz.x, xyz.y, xyz.z, A);
    if (mask) mask[at] = (uint8_t)m;
}

}  // namespace th
