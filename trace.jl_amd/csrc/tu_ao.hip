// tu_ao.hip — ambient occlusion (trhip_render_ao): the path integrator's ray generation and the scene's closest-hit walk, k_ao_spawn (th_ao.h), the scene's any-hit walk in
// its accumulate mode with a per-ray reach, then the path integrator's film pass.
#include "th_camera.h"
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
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_render_ao: the per-sample buffers of %llu camera samples (%.1f GB) do not fit in free HBM as one batch (%.1f GB free); there are no bands here",
                        (unsigned long long)total_slots, need * 1e-9, free_gb);
    }
    for (int j = 0; j < 3; ++j)
        if (int rc = ensure(ctx, ctx->sq[j], Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->ao_tmax, Pphys * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->Lbuf, total_slots * sizeof(float4))) return rc;
    if (int rc = ensure_film_samples(ctx, ds, total_slots)) return rc;
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    hipStream_t st = ctx->stream;
    const ShadowQueue sq{(float4*)ctx->sq[0].p, (float4*)ctx->sq[1].p, (float4*)ctx->sq[2].p};
    float* tmax = (float*)ctx->ao_tmax.p;
    float4* L = (float4*)ctx->Lbuf.p;
    ctx->last_L_count = 0;  // (until this frame's radiance is complete)
    ctx->last_L_kind = 0;

    Timer tm(ctx, ctx->timing && stats);
    FrameEvents ev;
    if (int rc = camera_pass_trace(ctx, scene, sensor, seed, sample_offset, tm, ev, cp)) return rc;
    Counters* ctr = cp.ctr;
    tm.begin(2, st);
    hipLaunchKernelGGL(k_ao_spawn, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, scene->dev, (const float4*)scene->g->d_base_colour.p, cp.pq, sq, tmax, cp.cap, (const float4*)cp.hits,
                       (uint32_t)total_slots, prm->max_distance, prm->background, prm->flags & TRHIP_AO_ALBEDO, L, ctr);
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
    ctx->last_L_count = total_slots;
    ctx->last_L_layout = 0;
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
