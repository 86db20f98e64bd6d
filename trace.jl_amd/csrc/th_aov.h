// th_aov.h — first-hit feature buffers (include/tracehip.h, trhip_render_aov): the two kernels between the existing ray generation / closest-hit launches and the outputs.
//
//   k_aov_resolve   hit queue -> one 80-byte trhip_aov_sample per camera sample (the interaction rebuilt as k_hit_geometry rebuilds it, the material's id and base colour)
//   k_aov_gather    records -> the three filtered planes, with the film pass's reach arithmetic, weights and summation order (k_film_gather_block's structure)
//
// Neither evaluates a BSDF, a light or a transcendental function: plain Float32 loads, multiplies and adds.
#pragma once
#include "th_kernels.h"

namespace th {

constexpr uint32_t kAovWords = 5;  // float4 words per record: {t, prim, b1, b2} {p, material} {n, 0} {ns, 0} {albedo, 0}

// One camera sample per lane, in k_raygen's dense order (lane i of the batch sits at k_raygen's physical queue position and carries its sample-major slot in o.w, so a wave
// writes 64 consecutive records: 5 KB of whole lines from five 16-byte stores per lane).  The interaction comes from rebuild_shading with the hit's ray, exactly as in
// k_hit_geometry: same inputs, same functions, same values.  base: one float4 per material (SceneGeometry::base_colour).
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_aov_resolve(DeviceScene sc, const float4* __restrict__ base, PathQueue q, uint32_t cap, const float4* __restrict__ hits, uint32_t n,
                                                        float4* __restrict__ rec) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t w = i >> 6;
        const uint32_t phys = (w % kSeg) * cap + (w / kSeg) * 64u + (i & 63u);  // k_raygen's placement
        const float4 o4 = q.o[phys], d4 = q.d[phys], h4 = hits[phys];
        const uint32_t slot = __float_as_uint(o4.w);
        const int prim = __float_as_int(h4.y);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 r1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), r2 = zero, r3 = zero, r4 = zero;
        if (prim >= 0) {
            Shading sh;
            uint32_t material = PRIM_NO_MATERIAL;
            const bool ok = rebuild_shading(sc, prim, mk3(o4.x, o4.y, o4.z), mk3(d4.x, d4.y, d4.z), sh, material);
            const bool has_mat = material != PRIM_NO_MATERIAL;
            const int mid = has_mat ? (int)material : -1;
            if (ok) {
                r1 = make_float4(sh.p.x, sh.p.y, sh.p.z, __int_as_float(mid));
                r2 = make_float4(sh.ng.x, sh.ng.y, sh.ng.z, 0.0f);
                r3 = make_float4(sh.ns.x, sh.ns.y, sh.ns.z, 0.0f);
            } else {
                r1.w = __int_as_float(mid);  // (k_hit_geometry writes zeros for a hit it cannot rebuild; so does this)
            }
            if (has_mat) {
                const float4 b = base[material];
                r4 = make_float4(b.x, b.y, b.z, 0.0f);
            }
        }
        float4* out = rec + (size_t)kAovWords * slot;
        out[0] = h4;
        out[1] = r1;
        out[2] = r2;
        out[3] = r3;
        out[4] = r4;
    }
}

// The three planes of film pixel block BX x BY per thread.  Everything that decides WHICH samples reach a pixel and with WHAT weight is k_film_gather_block's, line for line
// (tiles in k order, FilmTile bounds, the sample's clamped pixel range, ceil for the x table index and floor for y, the table in LDS); per tile one partial sum per value,
// added to the pixel's total when the tile's merge touches the pixel.  What differs: the values (no radiance, no NaN rule, no XYZ conversion), and that a missing sample
// adds its weight to plane 0's .w alone.  out: [pixel][plane] float4.
template <int BX, int BY>
__global__ __launch_bounds__(kBlock) void k_aov_gather(const DeviceSensor* __restrict__ sep, const float* __restrict__ table, const float4* __restrict__ rec, const float2* __restrict__ pfilm,
                                                       uint32_t spp, float4* __restrict__ out) {
    const DeviceSensor& se = *sep;
    __shared__ float s_table[256];
    for (uint32_t t = threadIdx.x; t < 256u; t += kBlock) s_table[t] = table[t];
    __syncthreads();
    const uint32_t npix = (uint32_t)(se.sb_w * se.band_rows);
    const float rx = se.filter_radius[0], ry = se.filter_radius[1];
    const float inv_rx = 1.0f / rx, inv_ry = 1.0f / ry;
    const uint32_t nbx = ((uint32_t)se.film_w + BX - 1) / BX, nby = ((uint32_t)se.film_h + BY - 1) / BY;
    for (uint32_t bidx = blockIdx.x * kBlock + threadIdx.x; bidx < nbx * nby; bidx += gridDim.x * kBlock) {
        const int fy0 = (int)(bidx / nbx) * BY, fx0 = (int)(bidx - (bidx / nbx) * nbx) * BX;
        float X[BX], Y[BY];
        for (int i = 0; i < BX; ++i) X[i] = se.crop_min[0] + (float)(fx0 + i);
        for (int j = 0; j < BY; ++j) Y[j] = se.crop_min[1] + (float)(fy0 + j);
        const int sx_lo = max((int)__builtin_floorf(X[0] - 1.5f - rx), se.sb_min[0]), sx_hi = min((int)__builtin_ceilf(X[BX - 1] + rx + 0.5f), se.sb_max[0]);
        const int sy_lo = max((int)__builtin_floorf(Y[0] - 1.5f - ry), se.sb_min[1]), sy_hi = min((int)__builtin_ceilf(Y[BY - 1] + ry + 0.5f), se.sb_max[1]);
        // per pixel: a = (w albedo, w of all samples), b = (w ns, w of hitting samples), c = (w p, w t)
        float4 ta[BY][BX], tb[BY][BX], tc[BY][BX];
        for (int j = 0; j < BY; ++j)
            for (int i = 0; i < BX; ++i) ta[j][i] = tb[j][i] = tc[j][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (sx_lo <= sx_hi && sy_lo <= sy_hi) {
            const int ty_lo = max((sy_lo - se.sb_min[1]) >> 4, se.band_ty0), ty_hi = min((sy_hi - se.sb_min[1]) >> 4, se.band_ty1);
            const int tx_lo = (sx_lo - se.sb_min[0]) >> 4, tx_hi = (sx_hi - se.sb_min[0]) >> 4;
            for (int ty = ty_lo; ty <= ty_hi; ++ty)
                for (int tx = tx_lo; tx <= tx_hi; ++tx) {
                    float bx0, by0, bx1, by1;
                    film_tile_bounds(se, ty, tx, rx, ry, bx0, by0, bx1, by1);
                    const float tbx0 = (float)se.sb_min[0] + (float)tx * 16.0f, tby0 = (float)se.sb_min[1] + (float)ty * 16.0f;
                    const float tbx1 = jmin(tbx0 + 15.0f, (float)se.sb_max[0]), tby1 = jmin(tby0 + 15.0f, (float)se.sb_max[1]);
                    bool in_tile[BY][BX];  // merge_film_tile! touches the pixel (film.jl:182-193)
                    bool any_in = false;
                    for (int j = 0; j < BY; ++j)
                        for (int i = 0; i < BX; ++i) {
                            in_tile[j][i] = !(X[i] < bx0 || X[i] > bx1 || Y[j] < by0 || Y[j] > by1);
                            any_in = any_in || in_tile[j][i];
                        }
                    if (!any_in) continue;
                    float4 ca[BY][BX], cb[BY][BX], cc[BY][BX];
                    for (int j = 0; j < BY; ++j)
                        for (int i = 0; i < BX; ++i) ca[j][i] = cb[j][i] = cc[j][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    const int y0 = max(sy_lo, (int)tby0), y1 = min(sy_hi, (int)tby1);
                    const int x0 = max(sx_lo, (int)tbx0), x1 = min(sx_hi, (int)tbx1);
                    for (int sy = y0; sy <= y1; ++sy)
                        for (int sx = x0; sx <= x1; ++sx) {
                            const uint32_t pix = (uint32_t)(sy - se.band_y0) * (uint32_t)se.sb_w + (uint32_t)(sx - se.sb_min[0]);
                            auto splat = [&](float2 pf, float4 r0, float4 r1, float4 r3, float4 r4) {
                                const float dpx = pf.x - 0.5f, dpy = pf.y - 0.5f;
                                float p0x = __builtin_ceilf(dpx - rx), p0y = __builtin_ceilf(dpy - ry);
                                float p1x = __builtin_floorf(dpx + rx) + 1.0f, p1y = __builtin_floorf(dpy + ry) + 1.0f;
                                p0x = jmax(p0x, jmax(bx0, 1.0f));
                                p0y = jmax(p0y, jmax(by0, 1.0f));
                                p1x = jmin(p1x, bx1);
                                p1y = jmin(p1y, by1);
                                bool okx[BX], oky[BY];
                                bool anyx = false, anyy = false;
                                for (int i = 0; i < BX; ++i) {
                                    okx[i] = !(X[i] < p0x || X[i] > p1x);
                                    anyx = anyx || okx[i];
                                }
                                for (int j = 0; j < BY; ++j) {
                                    oky[j] = !(Y[j] < p0y || Y[j] > p1y);
                                    anyy = anyy || oky[j];
                                }
                                if (!(anyx && anyy)) return;
                                const bool hit = __float_as_int(r0.y) >= 0;
                                int ox[BX], oy[BY];
                                for (int i = 0; i < BX; ++i) ox[i] = (int)jclamp(__builtin_ceilf(fabs_((X[i] - dpx) * inv_rx * 16.0f)), 1.0f, 16.0f) - 1;          // ceil for x …
                                for (int j = 0; j < BY; ++j) oy[j] = ((int)jclamp(__builtin_floorf(fabs_((Y[j] - dpy) * inv_ry * 16.0f)), 1.0f, 16.0f) - 1) * 16;  // … floor for y (A.9)
                                for (int j = 0; j < BY; ++j)
                                    for (int i = 0; i < BX; ++i)
                                        if (okx[i] && oky[j]) {
                                            const float w = s_table[oy[j] + ox[i]];
                                            ca[j][i].w += w;
                                            if (hit) {
                                                ca[j][i].x += r4.x * w;
                                                ca[j][i].y += r4.y * w;
                                                ca[j][i].z += r4.z * w;
                                                cb[j][i].x += r3.x * w;
                                                cb[j][i].y += r3.y * w;
                                                cb[j][i].z += r3.z * w;
                                                cb[j][i].w += w;
                                                cc[j][i].x += r1.x * w;
                                                cc[j][i].y += r1.y * w;
                                                cc[j][i].z += r1.z * w;
                                                cc[j][i].w += r0.x * w;
                                            }
                                        }
                            };
                            constexpr uint32_t kU = 2;  // samples whose loads are in flight together
                            uint32_t s = 0;
                            for (; s + kU <= spp; s += kU) {
                                float2 pfv[kU];
                                float4 r0[kU], r1[kU], r3[kU], r4[kU];
#pragma unroll
                                for (uint32_t u = 0; u < kU; ++u) {
                                    const size_t at = (size_t)(s + u) * npix + pix;
                                    const float4* r = rec + (size_t)kAovWords * at;
                                    pfv[u] = pfilm[at];
                                    r0[u] = r[0];
                                    r1[u] = r[1];
                                    r3[u] = r[3];
                                    r4[u] = r[4];
                                }
#pragma unroll
                                for (uint32_t u = 0; u < kU; ++u) splat(pfv[u], r0[u], r1[u], r3[u], r4[u]);
                            }
                            for (; s < spp; ++s) {
                                const size_t at = (size_t)s * npix + pix;
                                const float4* r = rec + (size_t)kAovWords * at;
                                splat(pfilm[at], r[0], r[1], r[3], r[4]);
                            }
                        }
                    auto add4 = [](float4& t, const float4& c) {
                        t.x += c.x;
                        t.y += c.y;
                        t.z += c.z;
                        t.w += c.w;
                    };
                    for (int j = 0; j < BY; ++j)
                        for (int i = 0; i < BX; ++i)
                            if (in_tile[j][i]) {
                                add4(ta[j][i], ca[j][i]);
                                add4(tb[j][i], cb[j][i]);
                                add4(tc[j][i], cc[j][i]);
                            }
                }
        }
        for (int j = 0; j < BY; ++j)
            for (int i = 0; i < BX; ++i)
                if (fx0 + i < se.film_w && fy0 + j < se.film_h) {
                    float4* o = out + 3 * ((size_t)(fy0 + j) * (size_t)se.film_w + (size_t)(fx0 + i));
                    o[0] = ta[j][i];
                    o[1] = tb[j][i];
                    o[2] = tc[j][i];
                }
    }
}

}  // namespace th
