// th_sky.h — the sky-lit frame (include/tracehip.h, trhip_render_sky; docs/design/25-sky.md): trhip_render_ao's frame with two substitutions, so the one kernel between the
// closest-hit launch over the camera rays and the any-hit launch over the occlusion rays.
//
//   k_sky_spawn   k_ao_spawn's work (th_ao.h: the same samples, occlusion ray, queue entry and append), with
//                   the contribution of an occlusion ray  c = env_eval(wi) * scale   (times the base colour under TRHIP_SKY_ALBEDO; zero for a primitive without a material)
//                   a miss                                L = env_eval(d) * scale    (the camera ray's direction; 0 under TRHIP_SKY_HIDE_BACKGROUND)
//
// With cosine-distributed wi the pdf cancels cos / π, so c is the unbiased one-sample estimate of the direct diffuse lighting under the environment.
// k_ao_spawn is not edited and not shared: its instruction stream stays what it was.  The map is small (256^2 texels are 1 MiB): it stays in L2 and is gathered.
#pragma once
#include "th_env.h"

namespace th {

// The lane-to-sample mapping, the segment arithmetic and the wave-aggregated append are k_ao_spawn's, comment for comment (th_ao.h).
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_sky_spawn(DeviceScene sc, const float4* __restrict__ base, PathQueue q, ShadowQueue sq, float* __restrict__ tmax, uint32_t cap,
                                                      const float4* __restrict__ hits, uint32_t n, float max_distance, DeviceEnv env, float scale, uint32_t albedo, uint32_t hide_background,
                                                      float4* __restrict__ L, Counters* ctr) {
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
            const f3 d = mk3(d4.x, d4.y, d4.z);
            f3 l0 = mk3(0.0f, 0.0f, 0.0f);
            if (prim >= 0) {
                const uint32_t key_hi = __float_as_uint(q.beta[phys].w);
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
                    const f3 e = env_eval(env, wi);
                    float4 c = make_float4(e.x * scale, e.y * scale, e.z * scale, 0.0f);
                    if (albedo) {
                        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (material != PRIM_NO_MATERIAL) b = base[material];
                        c = make_float4(c.x * b.x, c.y * b.y, c.z * b.z, 0.0f);
                    }
                    so4 = make_float4(org.x, org.y, org.z, o4.w);
                    sd4 = make_float4(cd.x, cd.y, cd.z, __uint_as_float(0u));  // no poison bits: texels and scale are finite and >= 0, so the contribution is never NaN
                    sc4 = c;
                    want = true;
                }
            } else if (!hide_background) {
                const f3 e = env_eval(env, d);
                l0 = mk3(e.x * scale, e.y * scale, e.z * scale);
            }
            L[__float_as_uint(o4.w)] = make_float4(l0.x, l0.y, l0.z, 0.0f);
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
