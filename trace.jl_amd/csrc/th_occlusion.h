// th_occlusion.h — the frame that tu_ao.hip and tu_sky.hip share: every camera ray to its first hit (th_camera.h), ONE spawn kernel that writes L[slot] for every sample and
// appends one occlusion ray per hit to the any-hit queue (origin | slot, direction, contribution, and its reach in ctx->ao_tmax beside the queue), the scene's any-hit walk in
// its accumulate mode with that per-ray reach, then the path integrator's film pass on the per-sample L.  One frame = one batch; there are no bands.
// The entry point checks its own parameter block and handles first (none of that needs a device) and passes its kernel launch as `spawn`; `who` names it in the refusal.
#pragma once
#include "th_camera.h"

// what a spawn kernel is launched with, beside its own parameters
struct OcclusionSpawn {
    hipStream_t st;
    int grid;
    const float4* base_colour;  // SceneGeometry::base_colour on the device
    PathQueue pq;               // the camera queue
    ShadowQueue sq;             // the any-hit queue
    float* tmax;                // the reach of every any-hit queue entry
    uint32_t cap;
    const float4* hits;
    uint32_t n;                 // camera samples
    float4* L;
    Counters* ctr;
};

template <class Spawn>
inline int occlusion_frame(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, const char* who, void* out,
                           bool out_is_device, trhip_stats* stats, Spawn&& spawn) {
    CameraPass cp;
    if (int rc = camera_pass_size(ctx, scene, sensor, spp, cp)) return rc;
    const DeviceSensor& ds = cp.ds;
    const uint64_t total_slots = cp.total_slots, Pphys = cp.Pphys;
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    {
        size_t held = ctx->hits.bytes + ctx->ao_tmax.bytes + ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->film_Lt.bytes + ctx->film.bytes;  // reused below
        for (int j = 0; j < 3; ++j) held += ctx->q[0][j].bytes + ctx->sq[j].bytes;
        // per physical queue entry: 3 + 1 + 3 float4 and the reach; per camera sample: the radiance, its re-laid copy (padded to whole pixel groups) and the film pass's side buffer
        const double need = (double)Pphys * (7.0 * sizeof(float4) + sizeof(float)) + (double)(total_slots + 64ull * spp) * 2.0 * sizeof(float4) + (double)total_slots * sizeof(uint4) +
                            (out_is_device ? 0.0 : (double)film_bytes) + 1.0e9;
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (Pphys >= (1ull << 31) || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "%s: the per-sample buffers of %llu camera samples (%.1f GB) do not fit in free HBM as one batch (%.1f GB free); there are no bands here", who,
                        (unsigned long long)total_slots, need * 1e-9, free_gb);
    }
    for (int j = 0; j < 3; ++j)
        if (int rc = ensure(ctx, ctx->sq[j], Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->ao_tmax, Pphys * sizeof(float))) return rc;
    ctx->last = LastRecords{};  // (until this frame's radiance is complete)
    if (int rc = ensure(ctx, ctx->Lbuf, total_slots * sizeof(float4))) return rc;
    if (int rc = ensure_film_samples(ctx, film_packed(ds), total_slots)) return rc;
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    hipStream_t st = ctx->stream;
    const ShadowQueue sq{(float4*)ctx->sq[0].p, (float4*)ctx->sq[1].p, (float4*)ctx->sq[2].p};
    float* tmax = (float*)ctx->ao_tmax.p;
    float4* L = (float4*)ctx->Lbuf.p;

    Timer tm(ctx, ctx->opt.timing && stats);
    FrameEvents ev;
    if (int rc = camera_pass_trace(ctx, scene, sensor, seed, sample_offset, tm, ev, cp)) return rc;
    Counters* ctr = cp.ctr;
    tm.begin(2, st);
    spawn(OcclusionSpawn{st, grid_for(ctx, total_slots, 8), (const float4*)scene->g->d_base_colour.p, cp.pq, sq, tmax, cp.cap, (const float4*)cp.hits, (uint32_t)total_slots, L, ctr});
    tm.end(2, st);
    tm.begin(3, st);
    // intersect_p with the per-ray reach; unoccluded rays add their contribution to L[slot] (the any-hit walk's accumulate mode)
    launch_trace(ctx, st, scene, true, SegQueue{ctr->n_shadow[0], cp.cap, 0u}, sq.o, sq.d, tmax, TraceOut{nullptr, L, sq.c, nullptr}, ctr->work_shadow[0], ctr);
    tm.end(3, st);
    tm.begin(4, st);
    launch_film(ctx, st, ds, cp.dsp, L, total_slots, spp, seed, sample_offset, (float4*)d_film, false);
    tm.end(4, st);
    HIP_TRY(ctx, ev.end(st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->last = LastRecords{total_slots, 0u, (uint32_t)((uint64_t)ds.sb_w * ds.sb_h), spp, 0u};
    if (int rc = copy_back(ctx, out, out_is_device, d_film, film_bytes)) return rc;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->camera_samples = total_slots;
        Counters h;
        HIP_TRY(ctx, hipMemcpy(&h, ctr, sizeof h, hipMemcpyDeviceToHost));
        stats_add_counters(*stats, h);
        stats_fill_times(ctx, scene, tm, ev, *stats);
        stats->n_batches = 1;
        stats->max_depth_reached = 1;
    }
    return 0;
}
