// th_path_env.h — the environment term of a path frame (include/tracehip.h, trhip_render_path_env; docs/design/26-path-env.md): a path that leaves the scene at depth d brings
// back beta * (E(dir) * scale), the last addend of its sample in depth order.  Neither k_shade_path nor a walk is touched: a miss is "nothing to shade" there, and its entry
// still sits in the depth's queue with its beta, its direction and its sample slot beside a hit record that says "miss".
//
//   k_path_escape   per depth, after the closest-hit walk has every ray's final answer and before the shade launch: every live entry whose hit record is a miss stores
//                   {beta.xyz, depth}, {dir.xyz, 0} at its sample's slot.  Plain vector stores, one writer per slot (a path escapes at most once), into a buffer zeroed at the
//                   start of the frame.  It never adds into L: the shadow rays of depth d - 1 may still be adding to the same slot on the second stream.
//   k_escape_fold   after the pipes have joined and k_apply_poison: out = base (all four lanes: in the fused layout .w is the film pass's descriptor), and where a record
//                   contributes  out.xyz = base.xyz + beta * (env_eval(dir) * scale)  — c = E * scale, t = beta * c, L' = L + t, one Float32 operation each.
//                   The base records stay as they are, so another environment folds over them without a walk (trhip_path_env_relight).
// Store once with plain stores, sum in a fixed order: the reproducible form of a scatter.
#pragma once
#include "th_env.h"

namespace th {

constexpr uint32_t kPathEnvHideBackground = 1u;  // TRHIP_PATH_ENV_HIDE_BACKGROUND

// Walks the segmented queue as k_shade_path does (seg_load, seg_locate_from, whole waves).  rec holds two float4 per slot; a slot is below the frame's record count by
// k_raygen's construction, as for L.
template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_path_escape(const uint32_t* __restrict__ counts, uint32_t cap, PathQueue qin, const float4* __restrict__ hits, uint32_t depth, float4* __restrict__ rec) {
    __shared__ SegView sv;
    const SegQueue qv{counts, cap, 0u};
    seg_load(qv, sv);
    const uint32_t total = sv.prefix[kSeg];  // multiple of kSegGran: whole waves
    uint32_t seg_in = 0;
    for (uint32_t flat = blockIdx.x * kBlock + threadIdx.x; flat < total; flat += gridDim.x * kBlock) {
        uint32_t lb;
        seg_locate_from(sv, flat & ~63u, seg_in, lb);
        const uint32_t local = lb + (flat & 63u);
        if (local >= sv.count[seg_in]) continue;  // padding
        const uint32_t i = seg_in * cap + local;
        if (__float_as_int(hits[i].y) >= 0) continue;  // a hit: k_shade_path's
        const float4 o4 = qin.o[i], d4 = qin.d[i], b4 = qin.beta[i];
        const size_t slot = __float_as_uint(o4.w);
        rec[2 * slot] = make_float4(b4.x, b4.y, b4.z, (float)depth);
        rec[2 * slot + 1] = make_float4(d4.x, d4.y, d4.z, 0.0f);
    }
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_escape_fold(const float4* __restrict__ base, const float4* __restrict__ rec, uint64_t n, DeviceEnv env, float scale, uint32_t flags,
                                                        float4* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        float4 l = base[i];
        const float4 r0 = rec[2 * i];
        if (r0.w != 0.0f && !((flags & kPathEnvHideBackground) && r0.w == 1.0f)) {
            const float4 r1 = rec[2 * i + 1];
            const f3 e = env_eval(env, mk3(r1.x, r1.y, r1.z));
            const float cx = e.x * scale, cy = e.y * scale, cz = e.z * scale;
            const float tx = r0.x * cx, ty = r0.y * cy, tz = r0.z * cz;
            l.x = l.x + tx;
            l.y = l.y + ty;
            l.z = l.z + tz;
        }
        out[i] = l;
    }
}

// Read-back of the records (trhip_last_escapes): 8 floats per camera sample, sample-major whatever the records' layout (k_export_L's indexing)
template <int TH_ONE_COPY = 0>
__global__ void k_export_escapes(const float4* __restrict__ rec, uint64_t n, float4* __restrict__ out, uint32_t layout, uint32_t npix, uint32_t spp) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t at = layout ? film_index(1u, npix, spp, (uint32_t)(i / npix), (uint32_t)(i % npix)) : (size_t)i;
    out[2 * i] = rec[2 * at];
    out[2 * i + 1] = rec[2 * at + 1];
}

}  // namespace th
