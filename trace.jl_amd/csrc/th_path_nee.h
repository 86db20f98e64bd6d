// th_path_nee.h — next-event estimation of the environment map in path frames (include/tracehip.h, trhip_render_path_env_nee; docs/design/28-path-nee.md): the path-env
// frame (th_path_env.h) with one shadow ray towards the map at every vertex whose BSDF has a non-specular lobe, and without the escapes that follow such a vertex.
// Neither k_shade_path nor a walk is touched: the path itself is trhip_render_path's in every bit.
//
//   k_path_nee         per depth, where k_path_escape runs in a path-env frame (after the closest-hit walk has every ray's final answer, before the shade launch):
//                        a miss  stores the escape record as k_path_escape does, with the 8th float 1 where the vertex before was non-specular (the escape is suppressed);
//                        a hit   notes whether its BSDF has a non-specular lobe (one byte per slot: one writer per slot and depth, plain stores, one stream) and, if it
//                                has, draws one direction from the one-sample mixture of BSDF sampling and map sampling and appends {origin, slot}, {direction, poison},
//                                {c} to the NEE shadow queue — to the input entry's own segment, so that a segment never receives more than `cap` entries.
//                      It never touches L: the shadow rays of depth d - 1 may still be adding to it.  The any-hit launch over the queue adds c where the ray is open.
//   k_escape_fold_nee  k_escape_fold (th_path_env.h) with the suppressed mark: a marked record contributes nothing.
#pragma once
#include "th_env_sample.h"
#include "th_path_env.h"

namespace th {

// The NEE shadow queues' counters: a buffer of their own beside Counters (whose layout stays), zeroed per batch.  First index = path depth - 1, second = segment * kCtrStride.
struct NeeCounters {
    uint32_t n[kMaxDepth + 2][kSeg * kCtrStride];     // NEE shadow rays emitted at that depth, per segment
    uint32_t work[kMaxDepth + 2][kSeg * kCtrStride];  // the any-hit launch's dynamic ray-fetch cursors
};

// One vertex's estimate (docs/design/28-path-nee.md "Definition", steps 2 - 9): true where a shadow ray is cast.  One Float32 operation per step.
TH_D bool nee_vertex(const LobeSet& bsdf, const Shading& sh, f3 wo, f3 beta, uint64_t key, uint32_t v, const DeviceEnv& env, const DeviceEnvSampler& smp, float scale, float mix, float om,
                     f3& org, f3& dir, f3& c) {
    constexpr int NS = BSDF_ALL & ~BSDF_SPECULAR;
    f3 wi;
    if (ts_uniform(key, ts_vertex_dim(v, TS_V_LIGHT_PICK)) < mix) {
        wi = env_sample(smp, env.R, ts_uniform(key, ts_vertex_dim(v, TS_V_LIGHT_U0)), ts_uniform(key, ts_vertex_dim(v, TS_V_LIGHT_U1)));
    } else {  // only the direction is taken from the sample
        const BsdfSample s = bsdf_sample_f(bsdf, sh, wo, f2{ts_uniform(key, ts_vertex_dim(v, TS_V_SCATTER_U0)), ts_uniform(key, ts_vertex_dim(v, TS_V_SCATTER_U1))}, NS);
        if (s.pdf == 0.0f) return false;
        wi = s.wi;
    }
    const float pb = bsdf_pdf(bsdf, sh, wo, wi, NS);
    const float pe = env_pdf(smp, env.R, wi);  // both densities always from the direction
    const float p = om * pb + mix * pe;
    if (!(p > 0.0f)) return false;
    const f3 fa = bsdf_f(bsdf, sh, wo, wi, NS) * fabs_(dot(wi, sh.ns));
    if (is_black(fa)) return false;
    const f3 e = env_eval(env, wi);
    const f3 ce = mk3(e.x * scale, e.y * scale, e.z * scale);
    const f3 t = fa * ce;
    const f3 Ld = t / p;
    c = beta * Ld;
    org = sh.p + 1e-6f * wi;     // spawn_ray(si, wi) Trace.jl:206-211
    dir = check_direction(wi);  // intersect_p(bvh, ray) starts with check_direction! (bvh.jl:265)
    return true;
}

// Walks the segmented queue as k_path_escape does (seg_load, seg_locate_from, whole waves: `total` is a multiple of 64 and no lane leaves the loop body early, so the
// append's ballot sees every lane).  The marginal's n + 1 floats are staged once per block in dynamic LDS, as in k_sky_spawn_is.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_path_nee(DeviceScene sc, const uint32_t* __restrict__ counts, uint32_t cap, PathQueue qin, const float4* __restrict__ hits, uint32_t depth,
                                                     uint32_t hits_have_bary, float4* __restrict__ rec, uint8_t* __restrict__ note, DeviceEnv env, DeviceEnvSampler smp, float scale, float mix,
                                                     float om, ShadowQueue nq, uint32_t* __restrict__ n_out) {
    extern __shared__ float s_marg[];
    __shared__ SegView sv;
    for (uint32_t k = threadIdx.x; k <= smp.n; k += kBlock) s_marg[k] = smp.marg[k];
    smp.marg = s_marg;
    const SegQueue qv{counts, cap, 0u};
    seg_load(qv, sv);  // (its barriers cover the staging above)
    const uint32_t total = sv.prefix[kSeg];
    uint32_t seg_in = 0;
    for (uint32_t flat = blockIdx.x * kBlock + threadIdx.x; flat < total; flat += gridDim.x * kBlock) {
        uint32_t lb;
        seg_locate_from(sv, flat & ~63u, seg_in, lb);
        const uint32_t local = lb + (flat & 63u);
        bool want = false;
        float4 so4, sd4, sc4;
        if (local < sv.count[seg_in]) {  // (else padding)
            const uint32_t i = seg_in * cap + local;
            const float4 h4 = hits[i];
            const int prim = __float_as_int(h4.y);
            const float4 o4 = qin.o[i], d4 = qin.d[i], b4 = qin.beta[i];
            const size_t slot = __float_as_uint(o4.w);
            if (prim < 0) {  // the escape record, marked where next-event estimation at the vertex before has already accounted for this light
                rec[2 * slot] = make_float4(b4.x, b4.y, b4.z, (float)depth);
                rec[2 * slot + 1] = make_float4(d4.x, d4.y, d4.z, note[slot] ? 1.0f : 0.0f);
            } else {
                const uint32_t meta = __float_as_uint(sc.shade[8 * (size_t)prim].w);
                bool non_specular = false;
                if (!(meta & PRIM_SPEC)) {  // (PRIM_SPEC: one perfectly specular lobe — the note alone, no shading rebuild and no material fetch)
                    const f3 d = mk3(d4.x, d4.y, d4.z);
                    Shading sh;
                    uint32_t material = PRIM_NO_MATERIAL;
                    if (rebuild_shading(sc, prim, mk3(o4.x, o4.y, o4.z), d, sh, material, hits_have_bary ? &h4 : nullptr) && material != PRIM_NO_MATERIAL) {
                        const LobeSet& bsdf = scene_materials(sc)[material].set[1];  // compute_scattering!(si, ray, true)
                        if (bsdf_has_non_specular(bsdf)) {
                            non_specular = true;
                            const f3 beta = mk3(b4.x, b4.y, b4.z);
                            const uint64_t key = ((uint64_t)__float_as_uint(b4.w) << 32) | (uint64_t)__float_as_uint(d4.w);  // the stream key travels with the path (k_raygen)
                            const uint32_t poison = ((isnan_(beta.x) || isinf_(beta.x)) ? 1u : 0u) | ((isnan_(beta.y) || isinf_(beta.y)) ? 2u : 0u) | ((isnan_(beta.z) || isinf_(beta.z)) ? 4u : 0u);
                            f3 org, dir, c;
                            if (nee_vertex(bsdf, sh, -d, beta, key, depth - 1u, env, smp, scale, mix, om, org, dir, c)) {
                                so4 = make_float4(org.x, org.y, org.z, o4.w);
                                sd4 = make_float4(dir.x, dir.y, dir.z, __uint_as_float(poison));
                                sc4 = make_float4(c.x, c.y, c.z, 0.0f);
                                want = true;
                            }
                        }
                    }
                }
                note[slot] = non_specular ? 1 : 0;
            }
        }
        const uint32_t si = seg_in * cap + wave_compact(want, &n_out[seg_in * kCtrStride]);
        if (want) {
            nq.o[si] = so4;
            nq.d[si] = sd4;
            nq.c[si] = sc4;
        }
    }
}

// k_escape_fold with the suppressed mark (rec[2 i + 1].w != 0: the escape follows a non-specular vertex and does not count)
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_escape_fold_nee(const float4* __restrict__ base, const float4* __restrict__ rec, uint64_t n, DeviceEnv env, float scale, uint32_t flags,
                                                            float4* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        float4 l = base[i];
        const float4 r0 = rec[2 * i];
        if (r0.w != 0.0f && !((flags & kPathEnvHideBackground) && r0.w == 1.0f)) {
            const float4 r1 = rec[2 * i + 1];
            if (r1.w == 0.0f) {
                const f3 e = env_eval(env, mk3(r1.x, r1.y, r1.z));
                const float cx = e.x * scale, cy = e.y * scale, cz = e.z * scale;
                const float tx = r0.x * cx, ty = r0.y * cy, tz = r0.z * cz;
                l.x = l.x + tx;
                l.y = l.y + ty;
                l.z = l.z + tz;
            }
        }
        out[i] = l;
    }
}

}  // namespace th
