// th_camera.h — the camera-ray front half that tu_aov.hip and the occlusion frames (th_occlusion.h: tu_ao.hip, tu_sky.hip) share: every camera ray of the frame in one queue (the path integrator's k_raygen), walked to its
// first hit.  camera_pass_size checks the scene, spp and the film and sizes the queue; the caller's fit check and its own buffers go between the two; camera_pass_trace uploads
// the sensor, grows the buffers, begins the frame's events and runs k_raygen and the closest-hit walk (Timer classes 0 and 1).
// A header of these two units, not a function of tu_path.hip or th_host.h: k_raygen is instantiated by the unit that launches it, so each unit's device code stays what it was.
#pragma once
#include "th_host.h"

struct CameraPass {
    DeviceSensor ds;
    const DeviceSensor* dsp;  // ds on the device
    PathQueue pq;             // ctx->q[0]
    float4* hits;
    Counters* ctr;
    uint32_t cap;             // entries per queue segment
    uint64_t Pphys;           // physical queue entries: kSeg segments of the capacity BEFORE it was narrowed to 32 bits (the caller refuses 2^31 and more)
    uint64_t total_slots;     // camera samples of the frame = rays in the queue
};
inline int camera_pass_size(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, CameraPass& cp) {
    if (!scene->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    if (spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    derive_sensor(sensor, cp.ds);
    if (cp.ds.film_w <= 0 || cp.ds.film_h <= 0 || cp.ds.sb_w <= 0 || cp.ds.sb_h <= 0) return fail(ctx, TRHIP_ERR_INVALID, "empty film");
    cp.total_slots = (uint64_t)cp.ds.sb_w * cp.ds.sb_h * spp;
    const uint64_t cap64 = queue_cap(cp.total_slots);  // the path integrator's physical queue layout (k_raygen)
    cp.cap = (uint32_t)cap64;
    cp.Pphys = cap64 * kSeg;
    return 0;
}
inline int camera_pass_trace(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint64_t seed, uint32_t sample_offset, Timer& tm, FrameEvents& ev, CameraPass& cp) {
    if (int rc = upload(ctx, ctx->sensor, &cp.ds, sizeof cp.ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
    for (int j = 0; j < 3; ++j)
        if (int rc = ensure(ctx, ctx->q[0][j], cp.Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->hits, cp.Pphys * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->counters, sizeof(Counters))) return rc;
    if (int rc = ensure_overflow(ctx)) return rc;
    hipStream_t st = ctx->stream;
    cp.dsp = (const DeviceSensor*)ctx->sensor.p;
    cp.pq = PathQueue{(float4*)ctx->q[0][0].p, (float4*)ctx->q[0][1].p, (float4*)ctx->q[0][2].p};
    cp.hits = (float4*)ctx->hits.p;
    cp.ctr = (Counters*)ctx->counters.p;
    HIP_TRY(ctx, ev.begin(st));
    HIP_TRY(ctx, hipMemsetAsync(cp.ctr, 0, sizeof(Counters), st));
    tm.begin(0, st);
    hipLaunchKernelGGL(k_raygen, dim3(grid_for(ctx, cp.total_slots, 8)), dim3(kBlock), 0, st, cp.dsp, 0u, (uint32_t)cp.total_slots, seed, sample_offset, cp.pq, cp.cap, cp.ctr, (float4*)nullptr, 0u,
                       FilmSideTable{nullptr, nullptr, 0});
    tm.end(0, st);
    tm.begin(1, st);
    // hits as the kernel-level entry point returns them ({t, prim, b1, b2}: bary_mode 0), through whatever walk the commit selected
    launch_trace(ctx, st, scene, false, SegQueue{cp.ctr->n_queue[0], cp.cap, 0u}, cp.pq.o, cp.pq.d, nullptr, TraceOut{cp.hits, nullptr, nullptr, nullptr, 0u, far_camera(scene, sensor) ? 1u : 0u},
                 cp.ctr->work_closest[0], cp.ctr);
    tm.end(1, st);
    return 0;
}
