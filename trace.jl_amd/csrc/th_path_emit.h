// th_path_emit.h — area lights in path frames (include/tracehip.h, trhip_emitters / trhip_render_path_emit; docs/design/29-path-emit.md): the triangles of chosen materials
// emit, a path that reaches one collects its light where no estimate has accounted for it, and every vertex with a non-specular BSDF casts one shadow ray towards a point
// drawn from the emitter set.  Neither k_shade_path nor a walk is touched: the path itself is trhip_render_path's in every bit.
//
//   emit_pick / emit_point   the sampler: xi -> emitter j (the fixed-trip search of th_env_sample.h over the cdf), (u0, u1) -> a point of triangle j
//   k_emitters_sample        count triples -> count (j, y, P_j / A_j)  (trhip_emitters_sample: the sampler on its own)
//   k_path_emit              per depth, where k_path_escape / k_path_nee run in their frames (after the closest-hit walk has every ray's final answer, before the shade launch).
//                              a miss  does nothing;
//                              a hit   adds beta * (Le * scale) to Lh[slot] where its material emits and the hit counts (one writer per slot and depth, plain loads and
//                                      stores, one stream), notes whether the vertex is specular (one byte per slot) and, at a non-specular vertex without HITS_ONLY, appends
//                                      {origin, slot}, {direction, poison}, {c} and the reach to the emitter shadow queue — to the input entry's own segment, so that a
//                                      segment never receives more than `cap` entries.
//                            It never touches L: the shadow rays of depth d - 1 may still be adding to it.  The any-hit launch over the queue adds c where the ray is open.
//   k_emit_fold              out = L + Lh, after the pipes have joined
//   k_export_emitted         Lh, sample-major whatever the records' layout (trhip_last_emitted)
//
// Device storage of an emitter set: 64 bytes per emissive triangle, {p0, P_j} {p1, A_j} {p2, as_float(slot)} {Le, 0}, emitters in ascending canonical slot; the cdf's n + 1
// floats; one float4 per material of the scene, Le or 0.
#pragma once
#include "th_env_sample.h"

namespace th {

struct DeviceEmitters {
    const float4* tri;     // 4 n
    const float* cdf;      // n + 1: cdf[0] = 0, cdf[n] = 1, monotone
    const float4* mat_le;  // one per material of the scene
    uint32_t n;
};
constexpr uint32_t kPathEmitHitsOnly = 1u;            // TRHIP_PATH_EMIT_HITS_ONLY
constexpr uint32_t kEmitCdfLdsBytes = 16u * 1024u;    // the cdf is staged per block in LDS when its n + 1 floats fit here (n <= 4095); a larger one is searched in global memory

// pick: the largest j in [0, n - 1] with cdf[j] <= xi.  A triangle without weight has cdf[j + 1] == cdf[j] and is never the largest such j.
__device__ inline uint32_t emit_pick(const float* __restrict__ cdf, uint32_t n, float xi) { return env_search(cdf, n, xi); }

// docs/design/29-path-emit.md "point", line by line
__device__ inline f3 emit_point(f3 p0, f3 p1, f3 p2, float u0, float u1) {
    const float s = sqrt_(u0);
    const float b0 = 1.0f - s;
    const float b1 = u1 * s;
    const float b2 = (1.0f - b0) - b1;
    return (b0 * p0 + b1 * p1) + b2 * p2;
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_emitters_sample(DeviceEmitters em, const float* __restrict__ u3, uint64_t count, uint32_t* __restrict__ out_index, float* __restrict__ out_point3,
                                                            float* __restrict__ out_pdf) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = emit_pick(em.cdf, em.n, u3[3 * i]);
        const float4 r0 = em.tri[4 * (size_t)j], r1 = em.tri[4 * (size_t)j + 1], r2 = em.tri[4 * (size_t)j + 2];
        const f3 y = emit_point(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), u3[3 * i + 1], u3[3 * i + 2]);
        out_index[i] = j;
        out_point3[3 * i] = y.x;
        out_point3[3 * i + 1] = y.y;
        out_point3[3 * i + 2] = y.z;
        out_pdf[i] = r0.w / r1.w;
    }
}

// One vertex's estimate (docs/design/29-path-emit.md "Definition", step 3): true where a shadow ray is cast.  One Float32 operation per step.
TH_D bool emit_vertex(const LobeSet& bsdf, const Shading& sh, f3 wo, f3 beta, uint64_t key, uint32_t v, const DeviceEmitters& em, const float* __restrict__ cdf, float scale, f3& org, f3& dir,
                      f3& c, float& reach) {
    constexpr int NS = BSDF_ALL & ~BSDF_SPECULAR;
    const uint32_t dim = (uint32_t)TS_DIM_EMIT_BASE + 3u * v;
    const float xi = ts_uniform(key, dim), u0 = ts_uniform(key, dim + 1u), u1 = ts_uniform(key, dim + 2u);
    const uint32_t j = emit_pick(cdf, em.n, xi);
    const float4 r0 = em.tri[4 * (size_t)j], r1 = em.tri[4 * (size_t)j + 1], r2 = em.tri[4 * (size_t)j + 2], r3 = em.tri[4 * (size_t)j + 3];
    const f3 p0 = mk3(r0.x, r0.y, r0.z), p1 = mk3(r1.x, r1.y, r1.z), p2 = mk3(r2.x, r2.y, r2.z);
    const f3 y = emit_point(p0, p1, p2, u0, u1);
    const f3 w = y - sh.p;
    const float d2 = dot(w, w);
    if (d2 == 0.0f) return false;
    const float dist = sqrt_(d2);
    const f3 wi = w / dist;
    const f3 nx = cross(p1 - p0, p2 - p0);
    const float nl = norm(nx);
    const f3 n_l = nx / nl;
    const float cl = fabs_(dot(n_l, wi));
    const float pa = r0.w / r1.w;  // P_j / A_j
    const float pn = pa * d2;
    const float pl = pn / cl;
    if (!(pl > 0.0f) || pl == kInf) return false;
    const f3 fa = bsdf_f(bsdf, sh, wo, wi, NS) * fabs_(dot(wi, sh.ns));
    if (is_black(fa)) return false;
    const f3 le = mk3(r3.x * scale, r3.y * scale, r3.z * scale);
    const f3 t = fa * le;
    const f3 Ld = t / pl;
    c = beta * Ld;
    org = sh.p + 1e-6f * wi;     // spawn_ray(si, wi) Trace.jl:206-211
    dir = check_direction(wi);  // intersect_p(bvh, ray) starts with check_direction! (bvh.jl:265)
    reach = dist * 0.999f;      // short of the emitter itself
    return true;
}

// Walks the segmented queue as k_path_nee does (seg_load, seg_locate_from, whole waves: `total` is a multiple of 64 and no lane leaves the loop body early, so the append's
// ballot sees every lane).  LDS_CDF: the cdf's n + 1 floats are staged once per block in dynamic LDS, as k_path_nee stages its marginal; otherwise the search reads em.cdf.
template <bool LDS_CDF>
__global__ __launch_bounds__(kBlock) void k_path_emit(DeviceScene sc, const uint32_t* __restrict__ counts, uint32_t cap, PathQueue qin, const float4* __restrict__ hits, uint32_t depth,
                                                      uint32_t hits_have_bary, float4* __restrict__ Lh, uint8_t* __restrict__ note, DeviceEmitters em, float scale, uint32_t flags,
                                                      ShadowQueue nq, float* __restrict__ ntmax, uint32_t* __restrict__ n_out) {
    extern __shared__ float s_cdf[];
    __shared__ SegView sv;
    const float* cdf = em.cdf;
    if (LDS_CDF) {
        for (uint32_t k = threadIdx.x; k <= em.n; k += kBlock) s_cdf[k] = em.cdf[k];
        cdf = s_cdf;
    }
    const SegQueue qv{counts, cap, 0u};
    seg_load(qv, sv);  // (its barriers cover the staging above)
    const uint32_t total = sv.prefix[kSeg];
    const bool hits_only = (flags & kPathEmitHitsOnly) != 0u;
    uint32_t seg_in = 0;
    for (uint32_t flat = blockIdx.x * kBlock + threadIdx.x; flat < total; flat += gridDim.x * kBlock) {
        uint32_t lb;
        seg_locate_from(sv, flat & ~63u, seg_in, lb);
        const uint32_t local = lb + (flat & 63u);
        bool want = false;
        float4 so4, sd4, sc4;
        float reach = 0.0f;
        if (local < sv.count[seg_in]) {  // (else padding)
            const uint32_t i = seg_in * cap + local;
            const float4 h4 = hits[i];
            const int prim = __float_as_int(h4.y);
            if (prim >= 0) {  // (a miss does nothing)
                const float4 o4 = qin.o[i], d4 = qin.d[i], b4 = qin.beta[i];
                const size_t slot = __float_as_uint(o4.w);
                const f3 beta = mk3(b4.x, b4.y, b4.z);
                const uint32_t meta = __float_as_uint(sc.shade[8 * (size_t)prim].w);
                const uint32_t mat = meta & PRIM_MATERIAL_MASK;
                // 1. the emitted term: the hit counts at depth 1, after a specular vertex, or under HITS_ONLY (elsewhere the vertex before has estimated this light)
                if (!(meta & PRIM_SPHERE) && mat < sc.n_materials) {
                    const float4 le = em.mat_le[mat];
                    if ((le.x != 0.0f || le.y != 0.0f || le.z != 0.0f) && (depth == 1u || hits_only || note[slot] != 0)) {
                        const float ex = le.x * scale, ey = le.y * scale, ez = le.z * scale;
                        const float tx = beta.x * ex, ty = beta.y * ey, tz = beta.z * ez;
                        float4 l = Lh[slot];
                        l.x = l.x + tx;
                        l.y = l.y + ty;
                        l.z = l.z + tz;
                        l.w = l.w + 1.0f;
                        Lh[slot] = l;
                    }
                }
                if (!hits_only) {
                    bool specular = true;
                    if (!(meta & PRIM_SPEC)) {  // (PRIM_SPEC: one perfectly specular lobe — the emitted term and the note alone, no shading rebuild and no material fetch)
                        const f3 d = mk3(d4.x, d4.y, d4.z);
                        Shading sh;
                        uint32_t material = PRIM_NO_MATERIAL;
                        if (rebuild_shading(sc, prim, mk3(o4.x, o4.y, o4.z), d, sh, material, hits_have_bary ? &h4 : nullptr) && material != PRIM_NO_MATERIAL) {
                            const LobeSet& bsdf = scene_materials(sc)[material].set[1];  // compute_scattering!(si, ray, true)
                            if (bsdf_has_non_specular(bsdf)) {
                                specular = false;
                                const uint64_t key = ((uint64_t)__float_as_uint(b4.w) << 32) | (uint64_t)__float_as_uint(d4.w);  // the stream key travels with the path (k_raygen)
                                const uint32_t poison = ((isnan_(beta.x) || isinf_(beta.x)) ? 1u : 0u) | ((isnan_(beta.y) || isinf_(beta.y)) ? 2u : 0u) | ((isnan_(beta.z) || isinf_(beta.z)) ? 4u : 0u);
                                f3 org, dir, c;
                                if (emit_vertex(bsdf, sh, -d, beta, key, depth - 1u, em, cdf, scale, org, dir, c, reach)) {
                                    so4 = make_float4(org.x, org.y, org.z, o4.w);
                                    sd4 = make_float4(dir.x, dir.y, dir.z, __uint_as_float(poison));
                                    sc4 = make_float4(c.x, c.y, c.z, 0.0f);
                                    want = true;
                                }
                            }
                        }
                    }
                    note[slot] = specular ? 1 : 0;
                }
            }
        }
        const uint32_t si = seg_in * cap + wave_compact(want, &n_out[seg_in * kCtrStride]);
        if (want) {
            nq.o[si] = so4;
            nq.d[si] = sd4;
            nq.c[si] = sc4;
            ntmax[si] = reach;
        }
    }
}

// out = L + Lh: the per-sample sum of the emitted terms joins the path's radiance once, after every depth (k_escape_fold's place and pattern)
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_emit_fold(const float4* __restrict__ base, const float4* __restrict__ Lh, uint64_t n, float4* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        float4 l = base[i];
        const float4 h = Lh[i];
        l.x = l.x + h.x;
        l.y = l.y + h.y;
        l.z = l.z + h.z;
        out[i] = l;
    }
}

// Read-back of Lh (trhip_last_emitted): 4 floats per camera sample, sample-major whatever the records' layout (k_export_L's indexing)
template <int TH_ONE_COPY = 0>
__global__ void k_export_emitted(const float4* __restrict__ Lh, uint64_t n, float4* __restrict__ out, uint32_t layout, uint32_t npix, uint32_t spp) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t at = layout ? film_index(1u, npix, spp, (uint32_t)(i / npix), (uint32_t)(i % npix)) : (size_t)i;
    out[i] = Lh[at];
}

}  // namespace th

// The object behind the opaque handle: the tables as uploaded; the host keeps nothing of the scene but the id of the geometry they were built from.
struct trhip_emitters {
    trhip_ctx* ctx = nullptr;
    uint64_t geometry_id = 0;
    uint32_t n = 0, n_materials = 0;
    DevBuf tri, cdf, mat_le;
    th::DeviceEmitters dev() const { return th::DeviceEmitters{(const float4*)tri.p, (const float*)cdf.p, (const float4*)mat_le.p, n}; }
};
