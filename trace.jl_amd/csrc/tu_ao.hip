// tu_ao.hip — ambient occlusion (trhip_render_ao): the path integrator's ray generation and the scene's closest-hit walk, k_ao_spawn (th_ao.h), the scene's any-hit walk in
// its accumulate mode with a per-ray reach, then the path integrator's film pass.
#include "th_host.h"
#include "th_ao.h"

namespace {

static_assert(sizeof(trhip_ao_params) == 16, "trhip_ao_params layout");

// One frame = one batch: the camera queue (o, d, key), its hits, the occlusion queue (o, d, contribution, reach) and the per-sample radiance are resident together.
int render_ao_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, const trhip_ao_params* prm, void* out,
                   bool out_is_device, trhip_stats* stats) {
    // the parameter block first: it is checked before any handle is looked at, and none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->max_distance > 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_ao: max_distance must be > 0 or +Inf");
    if (!(prm->background >= 0.0f) || std::isinf(prm->background)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_ao: background must be finite and >= 0");
    if (prm->flags & ~TRHIP_AO_ALBEDO) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_ao: unknown flag bits 0x%x", prm->flags & ~TRHIP_AO_ALBEDO);
    if (prm->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_ao: reserved must be 0");
    if (spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1");
    if (!ctx || !scene || !sensor || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!scene->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceSensor ds;
    derive_sensor(sensor, ds);
    if (ds.film_w <= 0 || ds.film_h <= 0 || ds.sb_w <= 0 || ds.sb_h <= 0) return fail(ctx, TRHIP_ERR_INVALID, "empty film");
    const uint64_t npix = (uint64_t)ds.sb_w * ds.sb_h;
    const uint64_t total_slots = npix * spp;
    const uint64_t P = total_slots;
    const uint64_t cap64 = ((P + kSeg - 1) / kSeg + 2 * kSegGran + kSegGran - 1) / kSegGran * kSegGran;  // the path integrator's physical queue layout (k_raygen)
    const uint64_t Pphys = cap64 * kSeg;
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        size_t held = ctx->hits.bytes + ctx->ao_tmax.bytes + ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->film_Lt.bytes + ctx->film.bytes;  // reused below
        for (int j = 0; j < 3; ++j) held += ctx->q[0][j].bytes + ctx->sq[j].bytes;
        // per physical queue entry: 3 + 1 + 3 float4 and the reach; per camera sample: the radiance, its re-laid copy (padded to whole pixel groups) and the film pass's side buffer
        const double need = (double)Pphys * (7.0 * sizeof(float4) + sizeof(float)) + (double)(total_slots + 64ull * spp) * 2.0 * sizeof(float4) + (double)total_slots * sizeof(uint4) +
                            (out_is_device ? 0.0 : (double)film_bytes) + 1.0e9;
        if (Pphys >= (1ull << 31) || need > 0.9 * (double)(free_b + held))
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_render_ao: the per-sample buffers of %llu camera samples (%.1f GB) do not fit in free HBM as one batch (%.1f GB free); there are no bands here",
                        (unsigned long long)total_slots, need * 1e-9, (double)(free_b + held) * 1e-9);
    }
    const uint32_t cap = (uint32_t)cap64;
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
    for (int j = 0; j < 3; ++j) {
        if (int rc = ensure(ctx, ctx->q[0][j], Pphys * sizeof(float4))) return rc;
        if (int rc = ensure(ctx, ctx->sq[j], Pphys * sizeof(float4))) return rc;
    }
    if (int rc = ensure(ctx, ctx->hits, Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->ao_tmax, Pphys * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->counters, sizeof(Counters))) return rc;
    if (int rc = ensure_overflow(ctx)) return rc;
    if (int rc = ensure(ctx, ctx->Lbuf, total_slots * sizeof(float4))) return rc;
    if (int rc = ensure_film_samples(ctx, ds, total_slots)) return rc;
    void* d_film = out;
    if (!out_is_device) {
        if (int rc = ensure(ctx, ctx->film, film_bytes)) return rc;
        d_film = ctx->film.p;
    }
    hipStream_t st = ctx->stream;
    const DeviceSensor* dsp = (const DeviceSensor*)ctx->sensor.p;
    Counters* ctr = (Counters*)ctx->counters.p;
    const PathQueue pq{(float4*)ctx->q[0][0].p, (float4*)ctx->q[0][1].p, (float4*)ctx->q[0][2].p};
    const ShadowQueue sq{(float4*)ctx->sq[0].p, (float4*)ctx->sq[1].p, (float4*)ctx->sq[2].p};
    float4* hits = (float4*)ctx->hits.p;
    float* tmax = (float*)ctx->ao_tmax.p;
    float4* L = (float4*)ctx->Lbuf.p;
    ctx->last_L_count = 0;  // (until this frame's radiance is complete)

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
    launch_trace(ctx, st, scene, false, SegQueue{ctr->n_queue[0], cap, 0u}, pq.o, pq.d, nullptr, TraceOut{hits, nullptr, nullptr, nullptr, 0u, far_camera(scene, sensor) ? 1u : 0u}, ctr->work_closest[0], ctr);
    tm.end(1, st);
    tm.begin(2, st);
    hipLaunchKernelGGL(k_ao_spawn, dim3(grid_for(ctx, P, 8)), dim3(kBlock), 0, st, scene->dev, (const float4*)scene->g->d_base_colour.p, pq, sq, tmax, cap, (const float4*)hits, (uint32_t)P,
                       prm->max_distance, prm->background, prm->flags & TRHIP_AO_ALBEDO, L, ctr);
    tm.end(2, st);
    tm.begin(3, st);
    // intersect_p with the per-ray reach; unoccluded rays add their contribution to L[slot] (the any-hit walk's accumulate mode)
    launch_trace(ctx, st, scene, true, SegQueue{ctr->n_shadow[0], cap, 0u}, sq.o, sq.d, tmax, TraceOut{nullptr, L, sq.c, nullptr}, ctr->work_shadow[0], ctr);
    tm.end(3, st);
    tm.begin(4, st);
    launch_film(ctx, st, ds, dsp, L, total_slots, spp, seed, sample_offset, (float4*)d_film, false);
    tm.end(4, st);
    HIP_TRY(ctx, hipEventRecord(e1, st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->last_L_count = total_slots;
    ctx->last_L_layout = 0;
    if (!out_is_device) HIP_TRY(ctx, hipMemcpy(out, d_film, film_bytes, hipMemcpyDeviceToHost));
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        Counters h;
        HIP_TRY(ctx, hipMemcpy(&h, ctr, sizeof h, hipMemcpyDeviceToHost));
        stats->camera_samples = total_slots;
        stats->closest_rays = h.closest_total;
        stats->shadow_rays = h.shadow_total;
        stats->nodes_visited = h.nodes_closest;
        stats->prims_tested = h.prims_closest;
        stats->nodes_visited_shadow = h.nodes_shadow;
        stats->prims_tested_shadow = h.prims_shadow;
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
        stats->ms_trace_any = tm.total(3, &stats->launches_trace_any);
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

int trhip_ao_default_params(trhip_ao_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    out->max_distance = kInf;
    out->background = 0.0f;
    out->flags = 0u;
    out->reserved = 0u;
    return 0;
}
int trhip_render_ao(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_ao_params* prm, float* out_xyzw, trhip_stats* st) {
    return render_ao_impl(ctx, sc, sn, spp, seed, off, prm, out_xyzw, false, st);
}
int trhip_render_ao_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_ao_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return render_ao_impl(ctx, sc, sn, spp, seed, off, prm, d_out_xyzw, true, st);
}

}  // extern "C"
