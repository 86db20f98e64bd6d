// th_sky_is.h — the importance-sampled sky frame (include/tracehip.h, trhip_render_sky_is; docs/design/27-sky-importance.md): trhip_render_sky's frame with one substitution
// per hit, so the one kernel between the closest-hit launch over the camera rays and the any-hit launch over the occlusion rays.
//
//   k_sky_spawn_is   k_sky_spawn's work (th_sky.h: the same samples, ray origin, queue entry and append, the same miss term), with
//                      the direction   wi = env_sample(u(LIGHT_U0), u(LIGHT_U1)) where u(LIGHT_PICK) < mix, the sky frame's cosine direction otherwise
//                      the weight      g = pc / ((1 - mix) pc + mix pe), pc = cos / π, pe = env_pdf(wi): the one-sample mixture estimator, g <= 1 / (1 - mix)
//                      the contribution of an occlusion ray  c = (env_eval(wi) * scale) * g   (times the base colour under TRHIP_SKY_ALBEDO)
//                    no ray where !(cos > 0) or !(p > 0): the sample keeps L = 0.
//
// k_sky_spawn and k_ao_spawn are not edited and not shared: their instruction streams stay what they were.  The tables are small ((n + 1)^2 floats: 258 KiB at 256^2) and stay in
// L2; the search is 2 ceil(log2 n) dependent loads per env-sampled lane, the marginal's half of them from a copy in LDS (measured against a search from global memory alone:
// spawn stage 0.50 against 0.54 ms on the probe, profiles/r24/sky_is.txt).
#pragma once
#include "th_env_sample.h"

namespace th {

// The lane-to-sample mapping, the segment arithmetic and the wave-aggregated append are k_ao_spawn's, comment for comment (th_ao.h).
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_sky_spawn_is(DeviceScene sc, const float4* __restrict__ base, PathQueue q, ShadowQueue sq, float* __restrict__ tmax, uint32_t cap,
                                                         const float4* __restrict__ hits, uint32_t n, float max_distance, DeviceEnv env, DeviceEnvSampler smp, float scale, float mix, float om,
                                                         uint32_t albedo, uint32_t hide_background, float4* __restrict__ L, Counters* ctr) {
    // the marginal's n + 1 floats, staged once per block (dynamic LDS, (n + 1) * 4 bytes: at most 16 KiB): its search and env_pdf's two reads then run from LDS
    extern __shared__ float s_marg[];
    for (uint32_t k = threadIdx.x; k <= smp.n; k += kBlock) s_marg[k] = smp.marg[k];
    __syncthreads();
    smp.marg = s_marg;
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
                    f3 wi;
                    if (ts_uniform(key, ts_vertex_dim(0u, TS_V_LIGHT_PICK)) < mix) {
                        wi = env_sample(smp, env.R, ts_uniform(key, ts_vertex_dim(0u, TS_V_LIGHT_U0)), ts_uniform(key, ts_vertex_dim(0u, TS_V_LIGHT_U1)));
                    } else {  // the sky frame's direction: the same numbers, the same arithmetic
                        f3 s, t;
                        coordinate_system(nf, s, t);
                        const f2 u{ts_uniform(key, ts_vertex_dim(0u, TS_V_BSDF_U0)), ts_uniform(key, ts_vertex_dim(0u, TS_V_BSDF_U1))};
                        const f3 wl = cosine_sample_hemisphere(u);
                        wi = (s * wl.x + t * wl.y) + nf * wl.z;
                    }
                    const float c0 = dot(nf, wi);
                    if (c0 > 0.0f) {
                        const float pc = c0 * kInvPi;
                        const float pe = env_pdf(smp, env.R, wi);  // always from the direction, never carried over from the sampling
                        const float p = om * pc + mix * pe;
                        if (p > 0.0f) {
                            const float g = pc / p;
                            const f3 org = sh.p + 1e-6f * wi;  // spawn_ray(si, wi) Trace.jl:206-211
                            const f3 cd = check_direction(wi);  // intersect_p(bvh, ray) starts with check_direction! (bvh.jl:265)
                            const f3 e = env_eval(env, wi);
                            float4 c = make_float4((e.x * scale) * g, (e.y * scale) * g, (e.z * scale) * g, 0.0f);
                            if (albedo) {
                                float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                                if (material != PRIM_NO_MATERIAL) b = base[material];
                                c = make_float4(c.x * b.x, c.y * b.y, c.z * b.z, 0.0f);
                            }
                            so4 = make_float4(org.x, org.y, org.z, o4.w);
                            sd4 = make_float4(cd.x, cd.y, cd.z, __uint_as_float(0u));  // no poison bits: E * scale / (1 - mix) is finite (the entry point checks it) and g <= 1 / (1 - mix)
                            sc4 = c;
                            want = true;
                        }
                    }
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
