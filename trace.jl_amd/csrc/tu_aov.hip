// tu_aov.hip — first-hit feature buffers (trhip_render_aov): the path integrator's ray generation and the scene's closest-hit walk, then k_aov_resolve and k_aov_gather (th_aov.h);
// trhip_render_aov_ids: the same frame with k_aov_ids (th_aov_ids.h) behind it.
#include "th_camera.h"
#include "th_aov.h"
#include "th_aov_ids.h"

namespace {

static_assert(sizeof(trhip_aov_sample) == kAovWords * sizeof(float4), "trhip_aov_sample layout");
static_assert(sizeof(trhip_aov_id) == sizeof(int4) && offsetof(trhip_aov_id, material) == 4 && offsetof(trhip_aov_id, t) == 8 && offsetof(trhip_aov_id, n_hit) == 12, "trhip_aov_id layout");
static_assert(offsetof(trhip_aov_sample, p) == 16 && offsetof(trhip_aov_sample, n) == 32 && offsetof(trhip_aov_sample, ns) == 48 && offsetof(trhip_aov_sample, albedo) == 64, "trhip_aov_sample layout");

constexpr int kAovBX = 1, kAovBY = 4;  // film pixels per thread of the gather (24 accumulators per pixel)

// One frame = one batch: the queue of every camera ray, its hit, its record and its film position are resident together (152 B per camera sample).
// with_ids: the call came through trhip_render_aov_ids (out_ids may still be NULL); otherwise out_ids is NULL and nothing below differs from what it was.
int render_aov_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, void* out_planes, void* out_samples,
                    void* out_ids, bool with_ids, bool out_is_device, trhip_stats* stats) {
    if (!ctx || !scene || !sensor) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!out_planes && !out_samples && !out_ids)
        return fail(ctx, TRHIP_ERR_INVALID, with_ids ? "trhip_render_aov_ids: all three output pointers are null" : "trhip_render_aov: both output pointers are null");
    CameraPass cp;
    if (int rc = camera_pass_size(ctx, scene, sensor, spp, cp)) return rc;
    ctx->last.drop_env_records();  // another render between a path-env frame and its relight: the relight is refused (include/tracehip.h, trhip_path_env_relight)
    const DeviceSensor& ds = cp.ds;
    const uint64_t total_slots = cp.total_slots;
    const size_t rec_bytes = (size_t)total_slots * sizeof(trhip_aov_sample);
    const size_t planes_bytes = (size_t)ds.film_w * ds.film_h * 3 * sizeof(float4);
    const bool rec_in_ctx = !(out_is_device && out_samples);
    const size_t ids_bytes = (size_t)ds.film_w * ds.film_h * sizeof(int4);
    const bool planes_in_ctx = out_planes && !out_is_device;
    const bool ids_in_ctx = out_ids && !out_is_device;
    {
        const size_t held = ctx->aov_rec.bytes + ctx->pfilm.bytes + ctx->hits.bytes + ctx->q[0][0].bytes + ctx->q[0][1].bytes + ctx->q[0][2].bytes + ctx->film.bytes;  // reused below
        const double need = (double)cp.Pphys * 4.0 * sizeof(float4) + (rec_in_ctx ? (double)rec_bytes : 0.0) + (out_planes ? (double)total_slots * sizeof(float2) : 0.0) +
                            (planes_in_ctx ? (double)planes_bytes : 0.0) + (ids_in_ctx ? (double)ids_bytes : 0.0) + 1.0e9;
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (cp.Pphys >= (1ull << 31) || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_render_aov: the per-sample buffers of %llu camera samples (%.1f GB) do not fit in free HBM as one batch (%.1f GB free); there are no bands here",
                        (unsigned long long)total_slots, need * 1e-9, free_gb);
    }
    float4* d_rec = (float4*)out_samples;
    if (rec_in_ctx) {
        if (int rc = ensure(ctx, ctx->aov_rec, rec_bytes)) return rc;
        d_rec = (float4*)ctx->aov_rec.p;
    }
    void* d_planes = out_planes;
    if (out_planes) {
        if (int rc = ensure(ctx, ctx->pfilm, total_slots * sizeof(float2))) return rc;
        if (int rc = stage_output(ctx, out_planes, out_is_device, planes_bytes + (ids_in_ctx ? ids_bytes : 0), &d_planes)) return rc;
    }
    void* d_ids = out_ids;
    if (ids_in_ctx) {  // the host variant's id plane lies behind its planes in the context's film buffer (planes_bytes is a multiple of 16)
        if (int rc = ensure(ctx, ctx->film, (planes_in_ctx ? planes_bytes : 0) + ids_bytes)) return rc;
        d_ids = (char*)ctx->film.p + (planes_in_ctx ? planes_bytes : 0);
    }
    hipStream_t st = ctx->stream;

    Timer tm(ctx, ctx->opt.timing && stats);
    FrameEvents ev;
    if (int rc = camera_pass_trace(ctx, scene, sensor, seed, sample_offset, tm, ev, cp)) return rc;
    tm.begin(2, st);
    hipLaunchKernelGGL(k_aov_resolve, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, scene->dev, (const float4*)scene->g->d_base_colour.p, cp.pq, cp.cap, (const float4*)cp.hits,
                       (uint32_t)total_slots, d_rec);
    tm.end(2, st);
    if (out_planes) {
        tm.begin(4, st);
        hipLaunchKernelGGL(k_film_positions, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, cp.dsp, total_slots, seed, sample_offset, (float2*)ctx->pfilm.p, 0u, spp);
        const uint64_t threads = (uint64_t)((ds.film_w + kAovBX - 1) / kAovBX) * (uint64_t)((ds.film_h + kAovBY - 1) / kAovBY);
        hipLaunchKernelGGL((k_aov_gather<kAovBX, kAovBY>), dim3(grid_for(ctx, threads, 8)), dim3(kBlock), 0, st, cp.dsp, (const float*)ctx->table.p, (const float4*)d_rec, (const float2*)ctx->pfilm.p, spp,
                           (float4*)d_planes);
        tm.end(4, st);
    }
    if (out_ids) {
        tm.begin(4, st);
        hipLaunchKernelGGL(k_aov_ids, dim3(grid_for(ctx, (uint64_t)ds.film_w * ds.film_h, 8)), dim3(kBlock), 0, st, cp.dsp, (const float4*)d_rec, spp, (int4*)d_ids);
        tm.end(4, st);
    }
    HIP_TRY(ctx, ev.end(st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (out_planes)
        if (int rc = copy_back(ctx, out_planes, out_is_device, d_planes, planes_bytes)) return rc;
    if (out_samples)
        if (int rc = copy_back(ctx, out_samples, out_is_device, d_rec, rec_bytes)) return rc;
    if (out_ids)
        if (int rc = copy_back(ctx, out_ids, out_is_device, d_ids, ids_bytes)) return rc;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->camera_samples = total_slots;
        Counters h;
        HIP_TRY(ctx, hipMemcpy(&h, cp.ctr, sizeof h, hipMemcpyDeviceToHost));
        stats_add_counters(*stats, h);
        stats_fill_times(ctx, scene, tm, ev, *stats);
        stats->n_batches = 1;
        stats->max_depth_reached = 1;
    }
    return 0;
}

}  // namespace

extern "C" {

int trhip_render_aov(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, float* out_planes, trhip_aov_sample* out_samples, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, out_planes, out_samples, nullptr, false, false, st);
}
int trhip_render_aov_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, void* d_out_planes, void* d_out_samples, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, d_out_planes, d_out_samples, nullptr, false, true, st);
}
int trhip_render_aov_ids(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, float* out_planes, trhip_aov_sample* out_samples,
                         trhip_aov_id* out_ids, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, out_planes, out_samples, out_ids, true, false, st);
}
int trhip_render_aov_ids_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, void* d_out_planes, void* d_out_samples,
                                void* d_out_ids, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, d_out_planes, d_out_samples, d_out_ids, true, true, st);
}

}  // extern "C"
