// th_ao.h — ambient occlusion (include/tracehip.h, trhip_render_ao; docs/design/13-ao.md): the one kernel between the existing closest-hit launch over the camera rays and the
// existing any-hit launch over the occlusion rays.
//
//   k_ao_spawn   hit queue -> L[slot] (the background on a miss, zero on a hit) and, for every hit whose interaction can be rebuilt, one any-hit queue entry:
//                origin | slot, direction | 0, contribution, and the ray's reach in the tmax array
//
// For a camera sample with stream key `key` whose camera ray (o, d) hits at p with shading normal ns (rebuild_shading, as k_aov_resolve and k_hit_geometry):
//   wo = -d,  nf = face_forward(ns, wo),  coordinate_system(nf, s, t)                                   (th_math.h, Trace.jl:139-146, :170)
//   u  = (ts_uniform(key, ts_vertex_dim(0, TS_V_BSDF_U0)), ts_uniform(key, ts_vertex_dim(0, TS_V_BSDF_U1)))   (the dimensions a path's first BSDF sample draws)
//   wl = cosine_sample_hemisphere(u)                                                                    (sqrt correctly rounded, sin / cos from trace_detmath.h)
//   wi = (s * wl.x + t * wl.y) + nf * wl.z        per component, in that order
//   occlusion ray = spawn_ray(si, wi) (Trace.jl:206-211) with a finite reach: o = p + 1e-6f * wi, d = wi, t_max = max_distance
// The any-hit launch (intersect_p) then adds the entry's contribution to L[slot] where the ray is unoccluded: 0 + c == c, one ray per slot, so nothing depends on order.
// The cosine pdf cancels cos / π: the contribution is 1, or the hit material's base colour (TRHIP_AO_ALBEDO; zero for a primitive without a material).
// The queue carries no time: scenes are static, the camera ray's time has nothing to act on.
#pragma once
#include "th_kernels.h"

namespace th {

// One camera sample per lane, in k_raygen's dense order (k_aov_resolve's phys / slot arithmetic).  Wave w of the dense index space sits in segment w % kSeg of the camera
// queue and appends to the SAME segment of the any-hit queue: a segment receives at most the entries its camera segment holds (<= cap), whatever the grid.  One ballot and
// one atomic per wave and 64 samples (wave_compact), as the path shading kernel appends its shadow rays.  The loop bound is rounded up to whole waves so that the ballot
// sees every lane.  base: one float4 per material (SceneGeometry::base_colour), read under TRHIP_AO_ALBEDO only.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_ao_spawn(DeviceScene sc, const float4* __restrict__ base, PathQueue q, ShadowQueue sq, float* __restrict__ tmax, uint32_t cap,
                                                     const float4* __restrict__ hits, uint32_t n, float max_distance, float background, uint32_t albedo, float4* __restrict__ L,
                                                     Counters* ctr) {
    const uint32_t n_up = (n + 63u) & ~63u;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_up; i += gridDim.x * kBlock) {
        const uint32_t w = i >> 6;
        const uint32_t seg = w % kSeg;
        const uint32_t phys = seg * cap + (w / kSeg) * 64u + (i & 63u);  // k_raygen's placement
        const bool valid = i < n;
        bool want = false;
        float4 so4, sd4, sc4;
        if (valid) {
            const float4 o4 = q.o[phys], d4 = q.d[phys], h4 = hits[phys];
            const int prim = __float_as_int(h4.y);
            float l0 = background;
            if (prim >= 0) {
                l0 = 0.0f;
                const uint32_t key_hi = __float_as_uint(q.beta[phys].w);
                const f3 d = mk3(d4.x, d4.y, d4.z);
                Shading sh;
                uint32_t material = PRIM_NO_MATERIAL;
                if (rebuild_shading(sc, prim, mk3(o4.x, o4.y, o4.z), d, sh, material)) {
                    const uint64_t key = ((uint64_t)key_hi << 32) | (uint64_t)__float_as_uint(d4.w);  // the stream key travels with the path (k_raygen)
                    const f3 nf = face_forward(sh.ns, -d);
                    f3 s, t;
                    coordinate_system(nf, s, t);
                    const f2 u{ts_uniform(key, ts_vertex_dim(0u, TS_V_BSDF_U0)), ts_uniform(key, ts_vertex_dim(0u, TS_V_BSDF_U1))};
                    const f3 wl = cosine_sample_hemisphere(u);
                    const f3 wi = (s * wl.x + t * wl.y) + nf * wl.z;
                    const f3 org = sh.p + 1e-6f * wi;  // spawn_ray(si, wi) Trace.jl:206-211
                    const f3 cd = check_direction(wi);  // intersect_p(bvh, ray) starts with check_direction! (bvh.jl:265)
                    float4 c = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
                    if (albedo) {
                        c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (material != PRIM_NO_MATERIAL) {
                            const float4 b = base[material];
                            c = make_float4(b.x, b.y, b.z, 0.0f);
                        }
                    }
                    so4 = make_float4(org.x, org.y, org.z, o4.w);
                    sd4 = make_float4(cd.x, cd.y, cd.z, __uint_as_float(0u));  // no poison bits: the contribution is finite
                    sc4 = c;
                    want = true;
                }
            }
            L[__float_as_uint(o4.w)] = make_float4(l0, l0, l0, 0.0f);
        }
        const uint32_t si = seg * cap + wave_compact(want, &ctr->n_shadow[0][seg * kCtrStride]);
        if (want) {
            sq.o[si] = so4;
            sq.d[si] = sd4;
            sq.c[si] = sc4;
            tmax[si] = max_distance;
        }
    }
}

}  // namespace th
