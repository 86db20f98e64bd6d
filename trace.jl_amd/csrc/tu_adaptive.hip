// tu_adaptive.hip — adaptive sampling beside the path frames (th_adaptive.h, docs/design/24-adaptive.md): the job list of a map frame (tu_path.hip renders it), and the two
// passes that turn a pilot frame's radiance records into a map: trhip_last_sample_stats and trhip_sample_map.
#include "th_host.h"
#include "th_adaptive.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

int map_job_list(trhip_ctx* ctx, uint32_t npix, uint32_t max_spp, bool sum_on_device, uint64_t* total, bool* above) {
    hipStream_t st = ctx->stream;
    const uint32_t* counts = (const uint32_t*)ctx->map_counts.p;
    if (sum_on_device) {  // Σ counts plans the batches on the host: the eight bytes this variant reads back
        if (int rc = ensure(ctx, ctx->map_word, sizeof(unsigned long long))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->map_word.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_map_reduce, dim3(grid_for(ctx, npix, 8)), dim3(kBlock), 0, st, counts, npix, max_spp, (unsigned long long*)ctx->map_word.p);
        unsigned long long word = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&word, ctx->map_word.p, sizeof word, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *above = (word & kMapAboveMax) != 0;
        *total = word & ~kMapAboveMax;
    }
    if (*above || *total == 0) return 0;
    if (int rc = ensure(ctx, ctx->map_offsets, (size_t)npix * sizeof(uint32_t))) return rc;
    if (int rc = ensure(ctx, ctx->map_jobs, (size_t)*total * sizeof(uint32_t))) return rc;
    size_t tmp_bytes = 0;
    HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, counts, (uint32_t*)ctx->map_offsets.p, (int)npix, st));
    if (int rc = ensure(ctx, ctx->map_tmp, tmp_bytes)) return rc;
    HIP_TRY(ctx, hipcub::DeviceScan::ExclusiveSum(ctx->map_tmp.p, tmp_bytes, counts, (uint32_t*)ctx->map_offsets.p, (int)npix, st));
    hipLaunchKernelGGL(k_map_expand, dim3(grid_for(ctx, npix, 8)), dim3(kBlock), 0, st, counts, (const uint32_t*)ctx->map_offsets.p, npix, (uint32_t*)ctx->map_jobs.p);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

namespace {

int stats_impl(trhip_ctx* ctx, void* out_mv, bool is_device) {
    if (!ctx || !out_mv) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (ctx->last.kind != 1 || ctx->last.count == 0)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_last_sample_stats: the context's last radiance records are not a one-band trhip_render_path frame's or trhip_film_accumulate's");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t npix = ctx->last.npix, spp = ctx->last.spp;
    const size_t bytes = (size_t)npix * sizeof(float2);
    void* d = out_mv;
    if (!is_device) {
        if (int rc = ensure(ctx, ctx->map_mv, bytes)) return rc;
        d = ctx->map_mv.p;
    }
    hipLaunchKernelGGL(k_sample_stats, dim3(grid_for(ctx, npix, 8)), dim3(kBlock), 0, ctx->stream, (const float4*)ctx->Lbuf.p, ctx->last.layout, npix, spp, (float2*)d);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!is_device) HIP_TRY(ctx, hipMemcpy(out_mv, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int map_impl(trhip_ctx* ctx, const void* mv, uint32_t sb_w, uint32_t sb_h, const trhip_sample_map_params* p, void* out_counts, void* out_total, bool is_device) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!p) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(p->tau > 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: tau must be > 0 (+Inf allowed)");
    if (!(std::isfinite(p->eps) && p->eps >= 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: eps must be finite and >= 0");
    if ((uint64_t)p->pilot + p->max_extra > (1u << 24)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: pilot + max_extra must be <= 2^24");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: unknown flag bits 0x%x", p->flags);
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: reserved must be 0");
    if (!ctx || !mv || !out_counts || !out_total) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (sb_w == 0 || sb_h == 0 || (uint64_t)sb_w * sb_h >= (1ull << 31)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_sample_map: %u x %u sample pixels", sb_w, sb_h);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t npix = sb_w * sb_h;
    const void* d_mv = mv;
    void *d_counts = out_counts, *d_total = out_total;
    if (!is_device) {
        if (int rc = upload(ctx, ctx->map_mv, mv, (size_t)npix * sizeof(float2))) return rc;
        if (int rc = ensure(ctx, ctx->map_out, (size_t)npix * sizeof(uint32_t))) return rc;
        if (int rc = ensure(ctx, ctx->map_word, sizeof(unsigned long long))) return rc;
        d_mv = ctx->map_mv.p;
        d_counts = ctx->map_out.p;
        d_total = ctx->map_word.p;
    }
    HIP_TRY(ctx, hipMemsetAsync(d_total, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_sample_map, dim3(grid_for(ctx, npix, 8)), dim3(kBlock), 0, ctx->stream, (const float2*)d_mv, sb_w, sb_h, SampleMapRule{p->tau, p->eps, p->pilot, p->max_extra}, (uint32_t*)d_counts,
                       (unsigned long long*)d_total);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!is_device) {
        HIP_TRY(ctx, hipMemcpy(out_counts, d_counts, (size_t)npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out_total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

int film_sum_impl(trhip_ctx* ctx, const void* a, const void* b, uint32_t width, uint32_t height, void* out, bool is_device) {
    if (!ctx || !a || !b || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_film_sum: empty film (%u x %u)", width, height);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n = (uint64_t)width * height;
    const size_t bytes = (size_t)n * sizeof(float4);
    const void *da = a, *db = b;
    void* d = out;
    if (!is_device) {  // the host variant's copies: a and b side by side, the sum over a
        if (int rc = ensure(ctx, ctx->map_mv, 2 * bytes)) return rc;
        da = d = ctx->map_mv.p;
        db = (const char*)ctx->map_mv.p + bytes;
        HIP_TRY(ctx, hipMemcpy(d, a, bytes, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy((char*)ctx->map_mv.p + bytes, b, bytes, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_film_sum, dim3(grid_for(ctx, n, 8)), dim3(kBlock), 0, ctx->stream, (const float4*)da, (const float4*)db, n, (float4*)d);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!is_device) HIP_TRY(ctx, hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int trhip_sample_map_default_params(trhip_sample_map_params* p) {
    if (!p) return TRHIP_ERR_INVALID;
    p->tau = 0.25f;
    p->eps = 0.01f;
    p->pilot = 8;
    p->max_extra = 56;
    p->flags = 0;
    p->reserved = 0;
    return 0;
}
int trhip_film_sum(trhip_ctx* ctx, const float* a, const float* b, uint32_t width, uint32_t height, float* out) { return film_sum_impl(ctx, a, b, width, height, out, false); }
int trhip_film_sum_device(trhip_ctx* ctx, const void* d_a, const void* d_b, uint32_t width, uint32_t height, void* d_out) { return film_sum_impl(ctx, d_a, d_b, width, height, d_out, true); }
int trhip_last_sample_stats(trhip_ctx* ctx, float* out_mv) { return stats_impl(ctx, out_mv, false); }
int trhip_last_sample_stats_device(trhip_ctx* ctx, void* d_out_mv) { return stats_impl(ctx, d_out_mv, true); }
int trhip_sample_map(trhip_ctx* ctx, const float* mv, uint32_t sb_width, uint32_t sb_height, const trhip_sample_map_params* params, uint32_t* out_counts, uint64_t* out_total) {
    return map_impl(ctx, mv, sb_width, sb_height, params, out_counts, out_total, false);
}
int trhip_sample_map_device(trhip_ctx* ctx, const void* d_mv, uint32_t sb_width, uint32_t sb_height, const trhip_sample_map_params* params, void* d_out_counts, void* d_out_total) {
    return map_impl(ctx, d_mv, sb_width, sb_height, params, d_out_counts, d_out_total, true);
}

}  // extern "C"
