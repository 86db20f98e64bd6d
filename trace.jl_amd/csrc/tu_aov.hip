// tu_aov.hip — first-hit feature buffers (trhip_render_aov): the path integrator's ray generation and the scene's closest-hit walk, then k_aov_resolve and k_aov_gather (th_aov.h).
#include "th_host.h"
#include "th_aov.h"

namespace {

static_assert(sizeof(trhip_aov_sample) == kAovWords * sizeof(float4), "trhip_aov_sample layout");
static_assert(offsetof(trhip_aov_sample, p) == 16 && offsetof(trhip_aov_sample, n) == 32 && offsetof(trhip_aov_sample, ns) == 48 && offsetof(trhip_aov_sample, albedo) == 64, "trhip_aov_sample layout");

constexpr int kAovBX = 1, kAovBY = 4;  // film pixels per thread of the gather (24 accumulators per pixel)

// One frame = one batch: the queue of every camera ray, its hit, its record and its film position are resident together (152 B per camera sample).
int render_aov_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, void* out_planes, void* out_samples,
                    bool out_is_device, trhip_stats* stats) {
    if (!ctx || !scene || !sensor) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!out_planes && !out_samples) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_aov: both output pointers are null");
    if (!scene->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    if (spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceSensor ds;
    derive_sensor(sensor, ds);
    if (ds.film_w <= 0 || ds.film_h <= 0 || ds.sb_w <= 0 || ds.sb_h <= 0) return fail(ctx, TRHIP_ERR_INVALID, "empty film");
    const uint64_t npix = (uint64_t)ds.sb_w * ds.sb_h;
    const uint64_t total_slots = npix * spp;
    const uint64_t P = total_slots;
    const uint64_t cap64 = ((P + kSeg - 1) / kSeg + 2 * kSegGran + kSegGran - 1) / kSegGran * kSegGran;  // the path integrator's physical queue layout (k_raygen)
    const uint64_t Pphys = cap64 * kSeg;
    const size_t rec_bytes = (size_t)total_slots * sizeof(trhip_aov_sample);
    const size_t planes_bytes = (size_t)ds.film_w * ds.film_h * 3 * sizeof(float4);
    const bool rec_in_ctx = !(out_is_device && out_samples);
    const bool planes_in_ctx = out_planes && !out_is_device;
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const size_t held = ctx->aov_rec.bytes + ctx->pfilm.bytes + ctx->hits.bytes + ctx->q[0][0].bytes + ctx->q[0][1].bytes + ctx->q[0][2].bytes + ctx->film.bytes;  // reused below
        const double need = (double)Pphys * 4.0 * sizeof(float4) + (rec_in_ctx ? (double)rec_bytes : 0.0) + (out_planes ? (double)total_slots * sizeof(float2) : 0.0) +
                            (planes_in_ctx ? (double)planes_bytes : 0.0) + 1.0e9;
        if (Pphys >= (1ull << 31) || need > 0.9 * (double)(free_b + held))
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_render_aov: the per-sample buffers of %llu camera samples (%.1f GB) do not fit in free HBM as one batch (%.1f GB free); there are no bands here",
                        (unsigned long long)total_slots, need * 1e-9, (double)(free_b + held) * 1e-9);
    }
    const uint32_t cap = (uint32_t)cap64;
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
    for (int j = 0; j < 3; ++j)
        if (int rc = ensure(ctx, ctx->q[0][j], Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->hits, Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->counters, sizeof(Counters))) return rc;
    if (int rc = ensure_overflow(ctx)) return rc;
    float4* d_rec = (float4*)out_samples;
    if (rec_in_ctx) {
        if (int rc = ensure(ctx, ctx->aov_rec, rec_bytes)) return rc;
        d_rec = (float4*)ctx->aov_rec.p;
    }
    float4* d_planes = (float4*)out_planes;
    if (out_planes) {
        if (int rc = ensure(ctx, ctx->pfilm, total_slots * sizeof(float2))) return rc;
        if (planes_in_ctx) {
            if (int rc = ensure(ctx, ctx->film, planes_bytes)) return rc;
            d_planes = (float4*)ctx->film.p;
        }
    }
    hipStream_t st = ctx->stream;
    const DeviceSensor* dsp = (const DeviceSensor*)ctx->sensor.p;
    Counters* ctr = (Counters*)ctx->counters.p;
    const PathQueue pq{(float4*)ctx->q[0][0].p, (float4*)ctx->q[0][1].p, (float4*)ctx->q[0][2].p};
    float4* hits = (float4*)ctx->hits.p;

    Timer tm(ctx, ctx->timing && stats);
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    HIP_TRY(ctx, hipEventRecord(e0, st));
    HIP_TRY(ctx, hipMemsetAsync(ctr, 0, sizeof(Counters), st));
    tm.begin(0, st);
    hipLaunchKernelGGL(k_raygen, dim3(grid_for(ctx, P, 8)), dim3(kBlock), 0, st, dsp, 0u, (uint32_t)P, seed, sample_offset, pq, cap, ctr, (float4*)nullptr, 0u, FilmSideTable{nullptr, nullptr, 0});
    tm.end(0, st);
    tm.begin(1, st);
    // hits as the kernel-level entry point returns them ({t, prim, b1, b2}: bary_mode 0), through whatever walk the commit selected
    launch_trace(ctx, st, scene, false, SegQueue{ctr->n_queue[0], cap, 0u}, pq.o, pq.d, nullptr, TraceOut{hits, nullptr, nullptr, nullptr, 0u, far_camera(scene, sensor) ? 1u : 0u}, ctr->work_closest[0], ctr);
    tm.end(1, st);
    tm.begin(2, st);
    hipLaunchKernelGGL(k_aov_resolve, dim3(grid_for(ctx, P, 8)), dim3(kBlock), 0, st, scene->dev, (const float4*)scene->g->d_base_colour.p, pq, cap, (const float4*)hits, (uint32_t)P, d_rec);
    tm.end(2, st);
    if (out_planes) {
        tm.begin(4, st);
        hipLaunchKernelGGL(k_film_positions, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, dsp, total_slots, seed, sample_offset, (float2*)ctx->pfilm.p, 0u, spp);
        const uint64_t threads = (uint64_t)((ds.film_w + kAovBX - 1) / kAovBX) * (uint64_t)((ds.film_h + kAovBY - 1) / kAovBY);
        hipLaunchKernelGGL((k_aov_gather<kAovBX, kAovBY>), dim3(grid_for(ctx, threads, 8)), dim3(kBlock), 0, st, dsp, (const float*)ctx->table.p, (const float4*)d_rec, (const float2*)ctx->pfilm.p, spp, d_planes);
        tm.end(4, st);
    }
    HIP_TRY(ctx, hipEventRecord(e1, st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (!out_is_device) {
        if (out_planes) HIP_TRY(ctx, hipMemcpy(out_planes, d_planes, planes_bytes, hipMemcpyDeviceToHost));
        if (out_samples) HIP_TRY(ctx, hipMemcpy(out_samples, d_rec, rec_bytes, hipMemcpyDeviceToHost));
    }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        Counters h;
        HIP_TRY(ctx, hipMemcpy(&h, ctr, sizeof h, hipMemcpyDeviceToHost));
        stats->camera_samples = total_slots;
        stats->closest_rays = h.closest_total;
        stats->nodes_visited = h.nodes_closest;
        stats->prims_tested = h.prims_closest;
        stats->fallback_rays = h.fallback_total;
        stats->nodes_visited_fallback = h.nodes_fallback;
        stats->prims_tested_fallback = h.prims_fallback;
        for (int k = 0; k < 4; ++k) stats->count_sub[k] = h.fallback_why[k];
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        stats->ms_total = ms;
        stats->ms_raygen = tm.total(0, &stats->launches_raygen);
        stats->ms_trace_closest = tm.total(1, &stats->launches_trace_closest);
        stats->ms_fallback = tm.fallback_total(&stats->launches_fallback);
        stats->ms_shade = tm.total(2, &stats->launches_shade);
        stats->ms_film = tm.total(4, &stats->launches_film);
        stats->n_batches = 1;
        stats->max_depth_reached = 1;
        traversal_info(ctx, scene, &stats->traversal, &stats->node_bytes);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
}

}  // namespace

extern "C" {

int trhip_render_aov(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, float* out_planes, trhip_aov_sample* out_samples, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, out_planes, out_samples, false, st);
}
int trhip_render_aov_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, void* d_out_planes, void* d_out_samples, trhip_stats* st) {
    return render_aov_impl(ctx, sc, sn, spp, seed, off, d_out_planes, d_out_samples, true, st);
}

}  // extern "C"
