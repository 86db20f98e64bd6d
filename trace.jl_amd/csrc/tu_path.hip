// tu_path.hip — PathIntegrator frames (classic per-depth wavefront, streaming wavefront, bands), the film pass, and the kernel-level entry
// points that use the shading / film kernels.
#include "th_host.h"
#include "th_adaptive.h"

// Film / sample-grid geometry derived from the sensor (film.jl:68-73, integrators/sampler.jl:13-20)
void derive_sensor(const trhip_sensor* sn, DeviceSensor& d) {
    std::memcpy(d.raster_to_camera, sn->raster_to_camera, sizeof d.raster_to_camera);
    std::memcpy(d.camera_to_world, sn->camera_to_world, sizeof d.camera_to_world);
    d.lens_radius = sn->lens_radius;
    d.focal_distance = sn->focal_distance;
    d.shutter_open = sn->shutter_open;
    d.shutter_close = sn->shutter_close;
    for (int i = 0; i < 2; ++i) {
        d.crop_min[i] = sn->crop_min[i];
        d.crop_max[i] = sn->crop_max[i];
        d.filter_radius[i] = sn->filter_radius[i];
        d.sb_min[i] = (int)std::floor(sn->crop_min[i] + 0.5f - sn->filter_radius[i]);
        d.sb_max[i] = (int)std::ceil(sn->crop_max[i] - 0.5f + sn->filter_radius[i]);
    }
    d.scale = sn->scale;
    d.sb_w = d.sb_max[0] - d.sb_min[0] + 1;
    d.sb_h = d.sb_max[1] - d.sb_min[1] + 1;
    d.film_w = (int)std::fabs(sn->crop_max[0] - (sn->crop_min[0] - 1.0f));  // inclusive_sides bounds.jl:100-102
    d.film_h = (int)std::fabs(sn->crop_max[1] - (sn->crop_min[1] - 1.0f));
    d.tiles_x = (int)std::floor(((float)(d.sb_max[0] - d.sb_min[0]) + 16.0f) / 16.0f);
    d.tiles_y = (int)std::floor(((float)(d.sb_max[1] - d.sb_min[1]) + 16.0f) / 16.0f);
    d.band_y0 = d.sb_min[1];  // one band: the whole frame
    d.band_rows = d.sb_h;
    d.band_ty0 = 0;
    d.band_ty1 = d.tiles_y - 1;
    d.accumulate = 0;
}

// ---- the film pass (th_kernels.h "film") ----
// k_shade_path's scene arguments: the shading lines and this handle's lights by value, the geometry's cold record (written at commit) by pointer
static ShadeScene shade_scene(const trhip_scene* s) { return ShadeScene{s->dev.shade, s->dev.lights, s->dev.n_lights, (const ShadeCold*)s->g->d_shade_cold.p}; }
// Two passes, and the filter alone chooses.  Packed, both radii in (0, 1] — every scene of the reference uses LanczosSincFilter(Point2f(1f0), 3f0) —: a sample reaches <= 4
// columns / rows, its 30-bit splat descriptor rides in the .w lane of its radiance record, and a thread gathers 2 x 4 film pixels.  Wide, anything else: film positions
// beside sample-major records and the 1 x 4 block gather.
bool film_packed(const DeviceSensor& ds) { return std::fmax(ds.filter_radius[0], ds.filter_radius[1]) <= 1.0f && ds.filter_radius[0] > 0.0f && ds.filter_radius[1] > 0.0f; }
// what the film pass reads per camera sample: the 16-byte radiance record, and the wide pass its film position (8 B)
static double film_sample_bytes(bool packed) { return packed ? 16.0 : 24.0; }
int ensure_film_samples(trhip_ctx* ctx, bool packed, uint64_t total_slots) { return packed ? 0 : ensure(ctx, ctx->pfilm, total_slots * sizeof(float2)); }
// pixel-group-major records (th_kernels.h, film_index layout 1) of one band: whole groups of 64 sample pixels
static uint64_t film_padded_slots(const DeviceSensor& ds, uint32_t spp) { return (((uint64_t)ds.sb_w * ds.band_rows + 63u) / 64u) * 64u * spp; }
// can k_raygen write the radiance records in the packed pass's layout, descriptors included (th_kernels.h, k_raygen's Lf)?  Whole sample passes of one band, 32-bit indices.
// A map frame asks this alone: it is fused or wide, whatever the two options say.
static bool film_fusable(const DeviceSensor& ds, uint32_t spp) { return film_packed(ds) && film_padded_slots(ds, spp) < (1ull << 32); }
static bool film_fused(const trhip_ctx* ctx, const DeviceSensor& ds, uint32_t spp) { return ctx->opt.film_fused && ctx->opt.film_relayout && film_fusable(ds, spp); }
static FilmSideTable film_side_table(trhip_ctx* ctx, hipStream_t st, uint64_t total_slots, bool* ok) {
    // side table for the descriptors that do not fit 30 bits (one sample in ~4000 at 1024^2): entry 0 of film_side is the counter, the descriptors follow
    const uint32_t side_cap = (uint32_t)std::min<uint64_t>(total_slots / 16 + 65536, 0x7ffffff0ull);
    *ok = ensure(ctx, ctx->film_side, ((size_t)side_cap + 1) * sizeof(uint4)) == 0;
    if (!*ok) return FilmSideTable{nullptr, nullptr, 0};
    (void)hipMemsetAsync(ctx->film_side.p, 0, sizeof(uint4), st);
    return FilmSideTable{(uint4*)ctx->film_side.p + 1, (uint32_t*)ctx->film_side.p, side_cap};
}
// `fused`: k_raygen wrote the records re-laid and with their descriptors (its side table is ctx->film_side, reset before the frame's first launch).  `map`: a map frame
// (trhip_render_path_map) — `spp` is its max_spp, which lays the records out; the gather stops at counts[pix], and only the drawn samples have a film position.
void launch_film(trhip_ctx* ctx, hipStream_t st, const DeviceSensor& ds, const DeviceSensor* dsp, const float4* L, uint64_t total_slots, uint32_t spp, uint64_t seed, uint32_t sample_offset,
                 float4* d_film, bool fused, const MapFrame* map) {
    const float* tb = (const float*)ctx->table.p;
    const bool packed = fused || (!map && film_packed(ds));
    uint32_t layout = 0;  // of L: sample-major, or 1 = pixel-group-major
    if (fused) {
        layout = 1;
    } else if (packed) {
        // the descriptors go into the records' .w lanes — on the way into a pixel-group-major copy when there is room for one (option "film_relayout", default on)
        bool ok = false;
        const FilmSideTable side = film_side_table(ctx, st, total_slots, &ok);
        if (!ok) return;
        const uint32_t npix_b = (uint32_t)(ds.sb_w * ds.band_rows);
        const uint64_t padded = film_padded_slots(ds, spp);
        if (ctx->opt.film_relayout && total_slots == (uint64_t)npix_b * spp && ensure(ctx, ctx->film_Lt, padded * sizeof(float4)) == 0) {
            layout = 1;
            hipLaunchKernelGGL(k_film_pack_transpose, dim3(grid_for(ctx, padded, 8)), dim3(kBlock), 0, st, dsp, npix_b, spp, seed, sample_offset, L, (float4*)ctx->film_Lt.p, side);
            L = (const float4*)ctx->film_Lt.p;
        } else {
            hipLaunchKernelGGL(k_film_pack_w, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, dsp, total_slots, seed, sample_offset, const_cast<float4*>(L), side);
        }
    } else if (map) {
        hipLaunchKernelGGL(k_film_positions_map, dim3(grid_for(ctx, map->total, 8)), dim3(kBlock), 0, st, dsp, map->jobs, map->total, seed, sample_offset, (float2*)ctx->pfilm.p);
    } else {  // (layout 0: k_film_positions still takes a layout, and spp to index the other one)
        hipLaunchKernelGGL(k_film_positions, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, st, dsp, total_slots, seed, sample_offset, (float2*)ctx->pfilm.p, 0u, spp);
    }
    const uint4* side_desc = ctx->film_side.p ? (const uint4*)ctx->film_side.p + 1 : nullptr;
    auto gather = [&](auto spp_arg) {  // the frame's spp, or a map frame's MapSpp
        using SPP = decltype(spp_arg);
        if (packed) {  // (xcd_bands 0: the kernel's workgroup swizzle lost its option)
            const uint64_t threads = (uint64_t)((ds.film_w + 1) / 2) * (uint64_t)((ds.film_h + 3) / 4);
            hipLaunchKernelGGL((k_film_gather_packed<2, 4, SPP>), dim3(grid_for(ctx, threads, 8)), dim3(kBlock), 0, st, dsp, tb, L, spp_arg, seed, sample_offset, layout, side_desc, d_film, 0u);
        } else {  // (layout 0: the block gather reads sample-major records and positions alone)
            const uint64_t threads = (uint64_t)ds.film_w * (uint64_t)((ds.film_h + 3) / 4);
            hipLaunchKernelGGL((k_film_gather_block<1, 4, SPP>), dim3(grid_for(ctx, threads, 8)), dim3(kBlock), 0, st, dsp, tb, L, (const float2*)ctx->pfilm.p, spp_arg, 0u, d_film);
        }
    };
    if (map)
        gather(MapSpp{map->counts, spp});
    else
        gather(spp);
}

// ---- the frame scaffold's out-of-line part (th_host.h) ----
void stats_add_counters(trhip_stats& s, const Counters& h) {
    s.closest_rays += h.closest_total;
    s.shadow_rays += h.shadow_total;
    s.nodes_visited += h.nodes_closest;
    s.prims_tested += h.prims_closest;
    s.nodes_visited_shadow += h.nodes_shadow;
    s.prims_tested_shadow += h.prims_shadow;
    s.fallback_rays += h.fallback_total;
    s.nodes_visited_fallback += h.nodes_fallback;
    s.prims_tested_fallback += h.prims_fallback;
    for (int k = 0; k < 4; ++k) s.count_sub[k] += h.fallback_why[k];
}
void stats_fill_times(trhip_ctx* ctx, const trhip_scene* sc, Timer& tm, const FrameEvents& ev, trhip_stats& s) {
    s.ms_total = ev.ms();
    s.ms_raygen = tm.total(0, &s.launches_raygen);
    s.ms_trace_closest = tm.total(1, &s.launches_trace_closest);
    s.ms_fallback = tm.fallback_total(&s.launches_fallback);
    s.ms_shade = tm.total(2, &s.launches_shade);
    s.ms_trace_any = tm.total(3, &s.launches_trace_any);
    s.ms_film = tm.total(4, &s.launches_film);
    traversal_info(ctx, sc, &s.traversal, &s.node_bytes);
}
void stats_accumulate(trhip_stats& sum, const trhip_stats& band) {
    sum.camera_samples += band.camera_samples;
    sum.closest_rays += band.closest_rays;
    sum.shadow_rays += band.shadow_rays;
    sum.nodes_visited += band.nodes_visited;
    sum.prims_tested += band.prims_tested;
    sum.nodes_visited_shadow += band.nodes_visited_shadow;
    sum.prims_tested_shadow += band.prims_tested_shadow;
    sum.fallback_rays += band.fallback_rays;
    sum.nodes_visited_fallback += band.nodes_visited_fallback;
    sum.prims_tested_fallback += band.prims_tested_fallback;
    for (int k = 0; k < 4; ++k) sum.count_sub[k] += band.count_sub[k];
    sum.ms_total += band.ms_total;
    sum.ms_raygen += band.ms_raygen;
    sum.ms_trace_closest += band.ms_trace_closest;
    sum.ms_fallback += band.ms_fallback;
    sum.ms_shade += band.ms_shade;
    sum.ms_trace_any += band.ms_trace_any;
    sum.ms_film += band.ms_film;
    sum.launches_raygen += band.launches_raygen;
    sum.launches_trace_closest += band.launches_trace_closest;
    sum.launches_fallback += band.launches_fallback;
    sum.launches_shade += band.launches_shade;
    sum.launches_trace_any += band.launches_trace_any;
    sum.launches_film += band.launches_film;
    sum.n_batches += band.n_batches;
    sum.max_depth_reached = band.max_depth_reached;
    sum.traversal = band.traversal;
    sum.node_bytes = band.node_bytes;
}

namespace {
// The queues, hit records, counters and overflow slabs of one pipe for `entries` physical queue entries (second_sq: the other parity's shadow queue of the two-stream mode).
int ensure_pipe_buffers(trhip_ctx* ctx, Pipe& pp, uint64_t entries, bool second_sq) {
    for (auto& a : pp.q)
        for (auto& b : a)
            if (int rc = ensure(ctx, b, entries * sizeof(float4))) return rc;
    for (auto& b : pp.sq)
        if (int rc = ensure(ctx, b, entries * sizeof(float4))) return rc;
    if (second_sq)
        for (auto& b : pp.sq2)
            if (int rc = ensure(ctx, b, entries * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, pp.hits, entries * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, pp.counters, sizeof(Counters))) return rc;
    const size_t slab_bytes = (size_t)trace_grid(ctx) * kBlock * (size_t)kStackSlabLevels * sizeof(uint2);
    for (auto& b : pp.overflow)
        if (int rc = ensure(ctx, b, slab_bytes)) return rc;
    return 0;
}
// The shade launch of both wavefronts: the scene picks the kernel's form (vertex tangents, a DirectionalLight).
template <bool STREAM>
void launch_shade_path(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const DeviceSensor* dsp, const PathQueue& in, const PathQueue& out, const ShadowQueue& sq, uint32_t cap,
                       const float4* hits, float4* L, Counters* ctr, int slot, int depth, int max_depth, uint32_t bary_mode, const ShadeStream& sst) {
    const dim3 grid(ctx->num_cu * 8), block(kBlock);
    if (has_directional_light(scene)) {
        if (scene->dev.tri_tan)
            hipLaunchKernelGGL((k_shade_path<STREAM, true, true>), grid, block, 0, st, shade_scene(scene), dsp, in, out, sq, cap, hits, L, ctr, slot, depth, max_depth, bary_mode, sst);
        else
            hipLaunchKernelGGL((k_shade_path<STREAM, false, true>), grid, block, 0, st, shade_scene(scene), dsp, in, out, sq, cap, hits, L, ctr, slot, depth, max_depth, bary_mode, sst);
    } else if (scene->dev.tri_tan) {
        hipLaunchKernelGGL(k_shade_path<STREAM>, grid, block, 0, st, shade_scene(scene), dsp, in, out, sq, cap, hits, L, ctr, slot, depth, max_depth, bary_mode, sst);
    } else {
        hipLaunchKernelGGL((k_shade_path<STREAM, false>), grid, block, 0, st, shade_scene(scene), dsp, in, out, sq, cap, hits, L, ctr, slot, depth, max_depth, bary_mode, sst);
    }
}
// PathIntegrator as a STREAMING wavefront (th_trace2.h "streaming wavefront"): rounds instead of depths.  A round
// traces every queued ray with a fetch budget, resumes the rays suspended in the round before, shades what finished (entries
// carry their own depth), and traces the shadow rays the same way.  max_depth + 16 budgeted rounds, then max_depth rounds
// without a budget, which complete whatever is left.  Radiance terms go to per-depth slots and are folded in depth order, so
// the per-sample radiance (and the film) is bit-identical to the classic per-depth wavefront.
int render_stream_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, const DeviceSensor& ds, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, void* out,
                       bool out_is_device, trhip_stats* stats, bool* declined) {
    *declined = true;
    const uint64_t npix = (uint64_t)ds.sb_w * ds.sb_h;
    const uint64_t total_slots = npix * spp;
    const int R_b = max_depth + 16, R = R_b + max_depth;
    if (R + 1 > kMaxDepth + 1) return 0;
    if ((uint64_t)max_depth * total_slots >= (1ull << 32)) return 0;
    if (total_slots >= (1ull << 31)) return 0;  // one batch: queue indices are 32-bit
    const uint64_t P = total_slots;
    const uint32_t list_cap = ctx->opt.stream_list_cap ? ctx->opt.stream_list_cap : (uint32_t)std::max<uint64_t>(65536, P / 128);
    const uint32_t cap = (uint32_t)queue_cap(P, list_cap / kSeg + 64);  // every segment keeps room for the resumed rays appended to it
    const uint64_t Pphys = (uint64_t)cap * kSeg;
    const size_t list_bytes = (size_t)list_cap * (4 * 16 + 16 + 4 + (size_t)kStack2Total * 8);
    const size_t terms_bytes = (size_t)max_depth * total_slots * sizeof(float4);
    const size_t need = terms_bytes + Pphys * (10 * 16 + 2 * 4) + 4 * list_bytes + total_slots * 24 + (3ull << 30);
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->st_terms.bytes + ctx->st_tags[0].bytes + ctx->st_tags[1].bytes;
        Pipe& p0 = ctx->pipes[0];
        held += p0.hits.bytes;
        for (auto& a : p0.q)
            for (auto& b : a) held += b.bytes;
        for (auto& b : p0.sq) held += b.bytes;
        for (auto& a : ctx->st_list)
            for (auto& b : a)
                for (auto& c : b) held += c.bytes;
        if ((double)need > 0.9 * (double)(free_b + held)) return 0;  // does not fit as one batch: the classic path cuts the frame into batches
    }
    *declined = false;
    Pipe& pp = ctx->pipes[0];
    if (int rc = ensure_pipe(ctx, 0, false)) return rc;
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
    if (int rc = ensure_pipe_buffers(ctx, pp, Pphys, false)) return rc;
    ctx->last = LastRecords{};
    if (int rc = ensure(ctx, ctx->Lbuf, total_slots * sizeof(float4))) return rc;
    if (int rc = ensure_film_samples(ctx, film_packed(ds), total_slots)) return rc;
    if (int rc = ensure(ctx, ctx->st_terms, terms_bytes)) return rc;
    for (int k = 0; k < 2; ++k)
        if (int rc = ensure(ctx, ctx->st_tags[k], Pphys * sizeof(uint32_t))) return rc;
    const size_t row_bytes = (size_t)kSeg * kCtrStride * sizeof(uint32_t);
    if (int rc = ensure(ctx, ctx->st_frozen, row_bytes)) return rc;
    if (int rc = ensure(ctx, ctx->st_counts, 16 * sizeof(uint32_t))) return rc;
    const size_t field_bytes[7] = {16, 16, 16, 16, 16, 4, (size_t)kStack2Total * 8};
    for (int kind = 0; kind < 2; ++kind)
        for (int pg = 0; pg < 2; ++pg)
            for (int f = 0; f < 7; ++f)
                if (int rc = ensure(ctx, ctx->st_list[kind][pg][f], (size_t)list_cap * field_bytes[f])) return rc;
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    auto list_of = [&](int kind, int pg) {
        DevBuf* b = ctx->st_list[kind][pg];
        return SuspendList{(float4*)b[0].p, (float4*)b[1].p, (float4*)b[2].p, (float4*)b[3].p, (uint4*)b[4].p, (uint32_t*)b[5].p, (uint2*)b[6].p, list_cap};
    };
    uint32_t* lc = (uint32_t*)ctx->st_counts.p;  // [0..1] closest list counts (ping-pong), [2] closest cursor, [4..5] any counts, [6] any cursor
    hipStream_t st = ctx->stream, ps = pp.st, ps2 = ctx->opt.overlap ? pp.st2 : pp.st;
    const DeviceSensor* dsp = (const DeviceSensor*)ctx->sensor.p;
    float4* L = (float4*)ctx->Lbuf.p;
    float4* terms = (float4*)ctx->st_terms.p;
    Counters* ctr = (Counters*)pp.counters.p;
    PathQueue pq[2];
    for (int k = 0; k < 2; ++k) pq[k] = PathQueue{(float4*)pp.q[k][0].p, (float4*)pp.q[k][1].p, (float4*)pp.q[k][2].p};
    uint32_t* tags[2] = {(uint32_t*)ctx->st_tags[0].p, (uint32_t*)ctx->st_tags[1].p};
    ShadowQueue sq{(float4*)pp.sq[0].p, (float4*)pp.sq[1].p, (float4*)pp.sq[2].p};
    float4* hits = (float4*)pp.hits.p;
    uint32_t* frozen = (uint32_t*)ctx->st_frozen.p;

    Timer tm(ctx, ctx->opt.timing && stats);
    FrameEvents ev;
    OwnedEvent ev_start;
    HIP_TRY(ctx, ev_start.create());
    HIP_TRY(ctx, ev.begin(st));
    HIP_TRY(ctx, hipMemsetAsync(terms, 0, terms_bytes, st));
    HIP_TRY(ctx, hipEventRecord(ev_start.e, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ps, ev_start.e, 0));
    HIP_TRY(ctx, hipMemsetAsync(ctr, 0, sizeof(Counters), ps));
    HIP_TRY(ctx, hipMemsetAsync(lc, 0, 16 * sizeof(uint32_t), ps));
    tm.begin(0, ps);
    hipLaunchKernelGGL(k_raygen, dim3(grid_for(ctx, P, 8)), dim3(kBlock), 0, ps, dsp, 0u, (uint32_t)P, seed, sample_offset, pq[0], cap, ctr);
    hipLaunchKernelGGL(k_fill_u32, dim3(grid_for(ctx, Pphys, 8)), dim3(kBlock), 0, ps, tags[0], Pphys, 1u);
    tm.end(0, ps);
    int cur = 0;
    for (int r = 0; r < R; ++r) {
        const uint32_t budget_min = r < R_b ? ctx->opt.stream_budget_min : 0u;  // the last max_depth rounds run every ray to its end
        const int in_pg = r & 1, out_pg = (r + 1) & 1;
        // ---- closest hits: fresh rays through frozen counts (finished resumed rays are appended to the live queue) ----
        HIP_TRY(ctx, hipMemcpyAsync(frozen, ctr->n_queue[r], row_bytes, hipMemcpyDeviceToDevice, ps));
        HIP_TRY(ctx, hipMemsetAsync(&lc[out_pg], 0, sizeof(uint32_t), ps));
        HIP_TRY(ctx, hipMemsetAsync(&lc[2], 0, sizeof(uint32_t), ps));
        StreamCtl sc_c{list_of(0, in_pg), list_of(0, out_pg), &lc[in_pg], &lc[2], &lc[out_pg], budget_min, ctx->opt.stream_budget_shift, pq[cur].beta, tags[cur], pq[cur].o, pq[cur].d, pq[cur].beta, hits, tags[cur],
                       ctr->n_queue[r], cap};
        const SegQueue qc{frozen, cap, 0u};
        const TraceOut oc{hits, nullptr, nullptr, nullptr, 1u};
        tm.begin(1, ps);
        launch_trace2_stream(ctx, ps, scene, false, qc, pq[cur].o, pq[cur].d, oc, ctr->work_closest[r], pp.overflow[0].p, ctr, sc_c);
        tm.end(1, ps);
        if (ps2 != ps && r > 0) HIP_TRY(ctx, hipStreamWaitEvent(ps, pp.ev_any, 0));  // shade(r) reuses the shadow queue
        tm.begin(2, ps);
        const ShadeStream sst{tags[cur], tags[cur ^ 1], (uint32_t)total_slots};
        launch_shade_path<true>(ctx, ps, scene, dsp, pq[cur], pq[cur ^ 1], sq, cap, hits, terms, ctr, r, 0, max_depth, 1u, sst);
        tm.end(2, ps);
        if (ps2 != ps) {
            HIP_TRY(ctx, hipEventRecord(pp.ev_shade, ps));
            HIP_TRY(ctx, hipStreamWaitEvent(ps2, pp.ev_shade, 0));
        }
        // ---- shadow rays: unoccluded ones add their contribution to the term slot ----
        HIP_TRY(ctx, hipMemsetAsync(&lc[4 + out_pg], 0, sizeof(uint32_t), ps2));
        HIP_TRY(ctx, hipMemsetAsync(&lc[6], 0, sizeof(uint32_t), ps2));
        StreamCtl sc_a{list_of(1, in_pg), list_of(1, out_pg), &lc[4 + in_pg], &lc[6], &lc[4 + out_pg], budget_min, ctx->opt.stream_budget_shift, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u};
        const SegQueue qa{ctr->n_shadow[r], cap, 0u};
        const TraceOut oa{nullptr, terms, sq.c, nullptr, 0u};
        tm.begin(3, ps2);
        launch_trace2_stream(ctx, ps2, scene, true, qa, sq.o, sq.d, oa, ctr->work_shadow[r], pp.overflow[1].p, ctr, sc_a);
        tm.end(3, ps2);
        if (ps2 != ps) HIP_TRY(ctx, hipEventRecord(pp.ev_any, ps2));
        cur ^= 1;
    }
    if (ps2 != ps) HIP_TRY(ctx, hipStreamWaitEvent(ps, pp.ev_any, 0));
    tm.begin(2, ps);
    hipLaunchKernelGGL(k_fold_terms, dim3(grid_for(ctx, total_slots, 8)), dim3(kBlock), 0, ps, (const float4*)terms, total_slots, (uint32_t)max_depth, L);
    tm.end(2, ps);
    HIP_TRY(ctx, hipEventRecord(pp.ev_done, ps));
    HIP_TRY(ctx, hipStreamWaitEvent(st, pp.ev_done, 0));
    tm.begin(4, st);
    // (no k_apply_poison here: the streaming shade kernel writes its terms — NaN included — straight into the per-depth slots and never notes
    //  poison; ctx->poison belongs to the classic path's two-stream mode alone)
    launch_film(ctx, st, ds, dsp, L, total_slots, spp, seed, sample_offset, (float4*)d_film, false);
    tm.end(4, st);
    HIP_TRY(ctx, ev.end(st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->last = LastRecords{total_slots, 0u, (uint32_t)npix, spp, 1u};
    if (int rc = copy_back(ctx, out, out_is_device, d_film, film_bytes)) return rc;
    uint32_t left[8];
    HIP_TRY(ctx, hipMemcpy(left, lc, sizeof left, hipMemcpyDeviceToHost));
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->camera_samples = total_slots;
        Counters h;
        HIP_TRY(ctx, hipMemcpy(&h, ctr, sizeof h, hipMemcpyDeviceToHost));
        stats_add_counters(*stats, h);
        stats_fill_times(ctx, scene, tm, ev, *stats);
        stats->n_batches = 1;
        stats->max_depth_reached = (uint32_t)max_depth;
    }
    if (left[R & 1] || left[4 + (R & 1)]) return fail(ctx, TRHIP_ERR_HIP, "streaming wavefront: %u + %u rays still suspended after the drain rounds", left[R & 1], left[4 + (R & 1)]);
    return 0;
}

// One band of a frame (band == nullptr: the whole frame, the normal case).  A band is a range of whole tile rows; its DeviceSensor carries
// the range and whether the film gather starts from zero or adds onto the bands before (th_scene.h).
int render_impl_band(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, int integrator, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, void* out,
                     bool out_is_device, trhip_stats* stats, const DeviceSensor* band, const MapFrame* map = nullptr, PathTerm* term = nullptr) {
    HostClock hclk;
    if (!ctx || !scene || !sensor || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!scene->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    if (integrator != 0 && integrator != 1) return fail(ctx, TRHIP_ERR_INVALID, "unknown integrator %d", integrator);
    // A GeometricPrimitive without a material makes the reference re-spawn the ray behind the hit without counting a bounce
    // (sppm.jl:219-222; Whitted calls a method that does not exist, sampler.jl:77-80).  The wavefront does not model that.
    if (scene->has_materialless_prim)  // found once, at commit: walking a million host records here cost 2.8 ms of every frame
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "rendering a scene with a material-less primitive is not supported (the trace entry points accept it)");
    if (spp == 0 || max_depth < 1 || max_depth > kMaxDepth) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1 and max_depth in 1..%d", kMaxDepth);
    if (!ctx->warned_idle_accelerator && ctx->opt.hybrid) {  // a two-tree scene rendered with options that leave its accelerator idle: said once per context (trhip_accelerator_note has it too)
        const char* why = hybrid_idle_reason(ctx, scene);
        if (why[0]) {
            ctx->warned_idle_accelerator = true;
            std::fprintf(stderr, "[tracehip] this scene holds the reference's tree and an accelerator, but the accelerator is idle: %s\n", why);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceSensor ds;
    if (band)
        ds = *band;
    else
        derive_sensor(sensor, ds);
    if (ds.film_w <= 0 || ds.film_h <= 0 || ds.sb_w <= 0 || ds.sb_h <= 0) return fail(ctx, TRHIP_ERR_INVALID, "empty film");
    const uint64_t npix = (uint64_t)ds.sb_w * ds.band_rows;
    const uint64_t total_slots = npix * spp;
    if (total_slots >= (1ull << 32)) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "more than 2^32 camera samples in one band of a frame");
    if (term)  // a term's refusals come after the path frame's
        if (int rc = term->check(ctx, scene)) return rc;
    if (integrator == 0) {
        if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
        if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
        ctx->last = LastRecords{};
        if (int rc = ensure(ctx, ctx->Lbuf, total_slots * sizeof(float4))) return rc;
        if (int rc = ensure_film_samples(ctx, film_packed(ds), total_slots)) return rc;
        if (int rc = ensure(ctx, ctx->counters, sizeof(Counters))) return rc;
        const size_t fb = (size_t)ds.film_w * ds.film_h * sizeof(float4);
        void* df;
        if (int rc = stage_output(ctx, out, out_is_device, fb, &df)) return rc;
        if (int rc = render_whitted_impl(ctx, scene, ds, sensor, spp, max_depth, seed, sample_offset, df, stats)) return rc;
        ctx->last = LastRecords{total_slots, 0u, (uint32_t)npix, spp, 0u};  // (render_whitted_impl has synchronised its stream)
        return copy_back(ctx, out, out_is_device, df, fb);
    }
    if (!band && !map && !term && (ctx->opt.streaming == 1 || (ctx->opt.streaming < 0 && total_slots <= 96ull * scene->g->prims.size())) && ctx->opt.traversal >= 2 && scene->wide_ok && scene->wide.root_cnt == 0 && scene->wide.root_ref != kRefNone && ctx->opt.batch_paths == 0 && ctx->opt.pipelines <= 1) {
        bool declined = false;
        const int rc = render_stream_impl(ctx, scene, sensor, ds, spp, max_depth, seed, sample_offset, out, out_is_device, stats, &declined);
        if (!declined) return rc;
    }
    // the radiance records: sample-major, or — when k_raygen can initialise them for the film pass — pixel-group-major, padded to whole groups of 64 pixels.
    // A map frame is fused or wide: one film pass per case, whatever the options "film_fused" / "film_relayout" say.
    const bool fused = map ? film_fusable(ds, spp) : film_fused(ctx, ds, spp);
    const bool packed = map ? fused : film_packed(ds);
    // A map frame (`spp` is its max_spp) has no bands: its records, dense at max_spp, with the poison byte, and the film pass's per-sample buffer must fit beside the queues.
    if (map) {
        bool fits = false;
        double free_gb = 0.0;
        const double need = (double)total_slots * (film_sample_bytes(packed) + 1.0) + (double)npix * 8.0 + (double)map->total * 4.0;
        if (int rc = fits_in_hbm(ctx, 2.0 * need, ctx->Lbuf.bytes + ctx->pfilm.bytes + held_in_pipes(ctx), &fits, &free_gb)) return rc;  // half of what is free, as render_impl plans its bands
        if (!fits) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers of a map frame (%.2f GB at max_spp %u) do not fit in half of free HBM (%.2f GB): there are no bands here", need * 1e-9, spp, free_gb);
    }
    // A frame with a term has no bands either: what the term's per-sample buffers need is the term's to refuse (film_own: an unfused film pass's buffer of its own)
    const double film_own = fused ? 0.0 : film_sample_bytes(packed);
    if (term)
        if (int rc = term->early_budget(ctx, total_slots, film_own, spp)) return rc;
    // wavefront batch = whole sample passes (a map frame: ranges of its job list); per path in flight: 2 x 3 queue float4 + 3 shadow float4 + 1 hit float4 = 160 B
    uint64_t batch_paths = ctx->opt.batch_paths;
    if (batch_paths == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + held_in_pipes(ctx);  // reused below, so it counts as available
        const double avail = 0.85 * (double)(free_b + held) - (double)total_slots * (sizeof(float4) + sizeof(float2)) - 2.5e9 - (term ? (double)total_slots * term->slot_bytes() : 0.0);
        // per path in flight: 2 x 3 queue float4 + 2 x 3 shadow float4 + 1 hit float4 + counters, and what the term's lane holds
        batch_paths = avail > 0 ? (uint64_t)(avail / (212.0 + (term ? term->path_bytes() : 0.0))) : npix;
    }
    uint64_t spp_batch = std::max<uint64_t>(1, batch_paths / npix);
    spp_batch = std::min<uint64_t>(spp_batch, spp);
    // Several batches run concurrently (one per pipeline): the memory budget is shared and the frame is cut into at
    // least `pipelines` batches when it has that many sample passes.
    const int want_pipes = map ? 1 : std::max(1, std::min(ctx->opt.pipelines, kMaxPipes));  // (a map frame ignores "pipelines")
    spp_batch = std::max<uint64_t>(1, std::min<uint64_t>(spp_batch / want_pipes, (spp + want_pipes - 1) / want_pipes));
    while (npix * spp_batch >= (1ull << 31)) spp_batch = (spp_batch + 1) / 2;  // queue indices are 32-bit
    const uint64_t total_jobs = map ? map->total : total_slots;  // the frame's camera samples: entries of the job list, or every slot
    uint64_t P = npix * spp_batch;
    if (map) {  // whole waves of jobs per batch; only the frame's last wave is partial
        P = std::min<uint64_t>(std::max<uint64_t>(64, batch_paths / 64 * 64), (total_jobs + 63) / 64 * 64);
        while (P >= (1ull << 31)) P = (P / 2 + 63) / 64 * 64;
    }
    const uint64_t n_batches_total = (total_jobs + P - 1) / P;
    const int NP = (int)std::min<uint64_t>(want_pipes, n_batches_total);
    const uint32_t cap = (uint32_t)queue_cap(P);
    const uint64_t Pphys = (uint64_t)cap * kSeg;
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sensor->filter_table, 256 * sizeof(float))) return rc;
    for (int pi = 0; pi < NP; ++pi) {
        if (int rc = ensure_pipe(ctx, pi, true)) return rc;
        if (int rc = ensure_pipe_buffers(ctx, ctx->pipes[pi], Pphys, ctx->opt.overlap)) return rc;
    }
    const uint64_t l_slots = fused ? film_padded_slots(ds, spp) : total_slots;
    ctx->last = LastRecords{};
    if (int rc = ensure(ctx, ctx->poison, l_slots)) return rc;
    if (int rc = ensure(ctx, ctx->Lbuf, l_slots * sizeof(float4))) return rc;
    if (term)  // its buffers, refused where they do not fit beside the frame's
        if (int rc = term->buffers(ctx, PathTermShape{NP, Pphys, total_slots, l_slots, film_own, spp})) return rc;
    if (int rc = ensure_film_samples(ctx, packed, total_slots)) return rc;
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    hipStream_t st = ctx->stream;
    const DeviceSensor* dsp = (const DeviceSensor*)ctx->sensor.p;
    float4* L = term ? term->base : (float4*)ctx->Lbuf.p;  // with a term the paths add into its base records, and Lbuf receives the term's fold

    hclk.tick("setup (budget, buffers)");
    Timer tm(ctx, ctx->opt.timing && stats);
    FrameEvents ev;
    OwnedEvent ev_start;
    HIP_TRY(ctx, ev_start.create());
    HIP_TRY(ctx, ev.begin(st));
    FilmSideTable fside{nullptr, nullptr, 0};
    if (fused) {
        bool ok = false;
        fside = film_side_table(ctx, st, total_slots, &ok);
        if (!ok) return fail(ctx, TRHIP_ERR_HIP, "the film pass's side table for %llu camera samples: %s", (unsigned long long)total_slots, ctx->err.c_str());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(L, 0, total_slots * sizeof(float4), st));
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->poison.p, 0, l_slots, st));
    if (term)
        if (int rc = term->clear(ctx, st, l_slots)) return rc;
    HIP_TRY(ctx, hipEventRecord(ev_start.e, st));
    const uint32_t bary_mode = (ctx->opt.traversal >= 2 && scene->wide_ok) ? 1u : 0u;  // k_trace2 hands the barycentrics to the shading kernel
    uint32_t n_batches = 0;
    for (int pi = 0; pi < NP; ++pi) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipes[pi].st, ev_start.e, 0));
        HIP_TRY(ctx, hipMemsetAsync(ctx->pipes[pi].counters.p, 0, sizeof(Counters), ctx->pipes[pi].st));
    }
    for (uint64_t j0 = 0; j0 < total_jobs; j0 += P) {  // (whole sample passes: j0 = s0 * npix)
        const int pipe = (int)(n_batches % NP);
        Pipe& pp = ctx->pipes[pipe];
        n_batches++;
        const uint64_t nb = std::min<uint64_t>(P, total_jobs - j0);
        // Within a batch, shadow rays of depth d (any-hit + accumulate) and closest-hit rays of depth d+1 are independent: two streams.
        hipStream_t ps = pp.st, ps2 = ctx->opt.overlap ? pp.st2 : pp.st;
        Counters* ctr = (Counters*)pp.counters.p;
        PathQueue pq[2];
        for (int k = 0; k < 2; ++k) pq[k] = PathQueue{(float4*)pp.q[k][0].p, (float4*)pp.q[k][1].p, (float4*)pp.q[k][2].p};
        // Two shadow queues, by parity of the depth: the shadow rays of depth d (low-priority stream, starved while the closest-hit rays of
        // depth d + 1 run) may go on while shade(d + 1) fills the other queue; shade(d + 2) waits for them.  They add into L, shade(d + 1)
        // only NOTES a non-finite beta in ctx->poison (k_apply_poison) — no two writers of one L entry at a time.  (One queue made every
        // shade launch wait for the shadow rays of the depth before: 2-6 ms each, 26 ms of the 436 ms S-mesh frame.)
        const bool two = ps2 != ps;
        const ShadowQueue sqs[2] = {ShadowQueue{(float4*)pp.sq[0].p, (float4*)pp.sq[1].p, (float4*)pp.sq[2].p},
                                    two ? ShadowQueue{(float4*)pp.sq2[0].p, (float4*)pp.sq2[1].p, (float4*)pp.sq2[2].p} : ShadowQueue{(float4*)pp.sq[0].p, (float4*)pp.sq[1].p, (float4*)pp.sq[2].p}};
        hipEvent_t ev_anys[2] = {pp.ev_any, pp.ev_any2};
        float4* hits = (float4*)pp.hits.p;
        HIP_TRY(ctx, hipMemsetAsync(ctr, 0, offsetof(Counters, closest_total), ps));  // queue sizes + work cursors of this batch
        if (term)
            if (int rc = term->begin_batch(ctx, ps, pipe)) return rc;
        tm.begin(0, ps);
        if (map)
            hipLaunchKernelGGL((k_raygen<0, MapJobs>), dim3(grid_for(ctx, nb, 8)), dim3(kBlock), 0, ps, dsp, MapJobs{map->jobs, (uint32_t)j0}, (uint32_t)nb, seed, sample_offset, pq[0], cap, ctr, fused ? L : nullptr, spp, fside);
        else
            hipLaunchKernelGGL(k_raygen, dim3(grid_for(ctx, nb, 8)), dim3(kBlock), 0, ps, dsp, (uint32_t)j0, (uint32_t)nb, seed, sample_offset, pq[0], cap, ctr, fused ? L : nullptr, spp, fside);
        tm.end(0, ps);
        int cur = 0;
        for (int depth = 1; depth <= max_depth; ++depth) {
            const ShadowQueue& sq = sqs[depth & 1];
            tm.begin(1, ps);
            launch_trace(ctx, ps, scene, false, SegQueue{ctr->n_queue[depth - 1], cap, 0u}, pq[cur].o, pq[cur].d, nullptr,
                         TraceOut{hits, nullptr, nullptr, nullptr, bary_mode, depth == 1 && far_camera(scene, sensor) ? 1u : 0u}, ctr->work_closest[depth - 1], ctr, pp.overflow[0].p);
            tm.end(1, ps);
            if (two && depth > 2) HIP_TRY(ctx, hipStreamWaitEvent(ps, ev_anys[depth & 1], 0));  // shade(d) refills the queue the shadow rays of depth d - 2 read
            tm.begin(2, ps);
            // every ray of this depth has its final answer: the term's kernel reads it (one writer per slot; never L, which the shadow rays of depth - 1 may still add to)
            if (term) term->after_closest(ctx, ps, scene, ctr->n_queue[depth - 1], cap, pq[cur], hits, depth, bary_mode, pipe);
            const ShadeStream sst{nullptr, nullptr, 0u, two ? (uint8_t*)ctx->poison.p : nullptr};
            launch_shade_path<false>(ctx, ps, scene, dsp, pq[cur], pq[cur ^ 1], sq, cap, hits, L, ctr, depth - 1, depth, max_depth, bary_mode, sst);
            tm.end(2, ps);
            if (two) {
                HIP_TRY(ctx, hipEventRecord(pp.ev_shade, ps));
                HIP_TRY(ctx, hipStreamWaitEvent(ps2, pp.ev_shade, 0));
            }
            tm.begin(3, ps2);
            launch_trace(ctx, ps2, scene, true, SegQueue{ctr->n_shadow[depth - 1], cap, 0u}, sq.o, sq.d, nullptr, TraceOut{nullptr, L, sq.c, nullptr}, ctr->work_shadow[depth - 1], ctr, pp.overflow[1].p);
            if (term) term->after_any(ctx, ps2, scene, cap, depth, pipe, ctr, pp.overflow[1].p);  // the term's rays of the same depth directly after, inside the same time class
            tm.end(3, ps2);
            if (two) HIP_TRY(ctx, hipEventRecord(ev_anys[depth & 1], ps2));
            cur ^= 1;
        }
        if (two) {  // the pipeline's next batch (or the film gather) needs every shadow ray resolved
            HIP_TRY(ctx, hipStreamWaitEvent(ps, ev_anys[max_depth & 1], 0));                       // the last depth's shadow rays
            if (max_depth >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ps, ev_anys[(max_depth - 1) & 1], 0));  // and the depth's before
        }
    }
    for (int pi = 0; pi < NP; ++pi) {
        HIP_TRY(ctx, hipEventRecord(ctx->pipes[pi].ev_done, ctx->pipes[pi].st));
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->pipes[pi].ev_done, 0));
    }
    tm.begin(4, st);
    if (ctx->opt.overlap) hipLaunchKernelGGL(k_apply_poison, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, L, (const uint8_t*)ctx->poison.p, l_slots);
    if (term) {  // (k_apply_poison above ran on the term's base records)
        L = (float4*)ctx->Lbuf.p;
        term->fold(ctx, st, l_slots, L);
    }
    launch_film(ctx, st, ds, dsp, L, total_slots, spp, seed, sample_offset, (float4*)d_film, fused, map);
    tm.end(4, st);
    HIP_TRY(ctx, ev.end(st));
    HIP_TRY(ctx, hipGetLastError());
    hclk.tick("enqueue");
    HIP_TRY(ctx, hipStreamSynchronize(st));
    hclk.tick("stream sync");
    ctx->last = LastRecords{total_slots, fused ? 1u : 0u, (uint32_t)npix, spp, map ? 2u : band ? 0u : 1u};
    if (term) {  // what the term leaves behind: its mark in ctx->last, and how the film pass ran where a later call repeats it
        PathEnvKeep k;
        k.ds = ds;
        std::memcpy(k.filter_table, sensor->filter_table, sizeof k.filter_table);
        k.spp = spp, k.sample_offset = sample_offset, k.seed = seed, k.total_slots = total_slots, k.l_slots = l_slots, k.fused = fused;
        term->retain(ctx, k);
    }
    if (int rc = copy_back(ctx, out, out_is_device, d_film, film_bytes)) return rc;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->camera_samples = total_jobs;
        for (int pi = 0; pi < NP; ++pi) {
            Counters h;
            HIP_TRY(ctx, hipMemcpy(&h, ctx->pipes[pi].counters.p, sizeof h, hipMemcpyDeviceToHost));
            stats_add_counters(*stats, h);
        }
        stats_fill_times(ctx, scene, tm, ev, *stats);
        stats->n_batches = n_batches;
        stats->max_depth_reached = (uint32_t)max_depth;
        // The certified walk's cliff: scenes made of near-ties (tiny coplanar triangles, rays in a wall's plane — tests/attack_scenes.py) send up to half of their rays to the
        // reference-order walk: exact, at about twice the closest-hit time.  Said once per context, and kept for trhip_accelerator_note.
        ctx->last_fallback_share = stats->closest_rays ? (double)stats->fallback_rays / (double)stats->closest_rays : 0.0;
        if (stats->traversal == 9 && ctx->last_fallback_share > 0.2 && !ctx->warned_fallback_cliff) {
            ctx->warned_fallback_cliff = true;
            std::fprintf(stderr, "[tracehip] the certified walk handed %.0f %% of this frame's closest-hit rays back to the reference-order walk (near-ties, grazed leaf boxes, rays in a "
                                 "primitive's plane): the frame is exact but the accelerator saves little on this scene\n", 100.0 * ctx->last_fallback_share);
        }
    }
    hclk.tick("counters + event times");
    return 0;
}

// Bands of a frame whose per-sample buffers do not fit (render_impl below): whole rows of 16 x 16 sample tiles, as many per band as `budget` bytes hold at `bytes_per_sample`
// (and fewer than 2^32 sample slots: 32-bit indices).  Host arithmetic only: trhip_plan_bands exposes it, tests/test_sharding_gloo.py checks C5's numbers on CPU.
int plan_rows_per_band(const DeviceSensor& ds, uint32_t spp, double budget_bytes, double bytes_per_sample) {
    const double row_bytes = (double)ds.sb_w * 16.0 * (double)spp * bytes_per_sample;
    int rows = (int)std::max(1.0, std::min((double)ds.tiles_y, std::floor(budget_bytes / row_bytes)));
    while (rows > 1 && (uint64_t)ds.sb_w * 16ull * (uint64_t)rows * spp >= (1ull << 32)) --rows;
    return rows;
}
DeviceSensor band_of(const DeviceSensor& ds, int t0, int rows_per_band) {
    DeviceSensor b = ds;
    b.band_ty0 = t0;
    b.band_ty1 = std::min(ds.tiles_y, t0 + rows_per_band) - 1;
    b.band_y0 = ds.sb_min[1] + 16 * t0;
    b.band_rows = std::min(ds.sb_max[1], ds.sb_min[1] + 16 * b.band_ty1 + 15) - b.band_y0 + 1;
    b.accumulate = t0 > 0 ? 1 : 0;
    return b;
}
// A frame: one band when its per-sample buffers (radiance 16 B + film position 8 B per camera sample) fit in HBM next to the queues — every
// BASELINE configuration up to 1024^2 x 256 spp does — otherwise bands of whole tile rows, rendered one after the other into the same film.
// The film is the sequential tile loop's bit for bit either way: a film pixel receives its tiles in k order (integrators/sampler.jl:24-52,
// film.jl:182-193), and bands are ranges of k.  (4096^2 x 1024 spp, BASELINE configs[4], is 412 GB of samples: 3 bands on one MI355X.)
int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, int integrator, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, void* out,
                bool out_is_device, trhip_stats* stats) {
    if (!ctx || !scene || !sensor || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    DeviceSensor ds;
    derive_sensor(sensor, ds);
    int rows_per_band = ds.tiles_y;  // in tile rows
    if (integrator == 1 && ds.sb_w > 0 && ds.sb_h > 0 && spp > 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (ctx->opt.band_tile_rows > 0) {
            rows_per_band = std::min<int>(ds.tiles_y, ctx->opt.band_tile_rows);
        } else {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
            const size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + held_in_pipes(ctx);
            // half of what is free for the per-sample buffers, the rest for the wavefront queues (164 B per path in flight); 32-bit slot indices
            const double budget = std::min(0.5 * (double)(free_b + held), 4.0e9 * 24.0);
            rows_per_band = plan_rows_per_band(ds, spp, budget, film_sample_bytes(film_packed(ds)) + 1.0);  // radiance (+ film position) + poison byte
        }
    }
    if (rows_per_band >= ds.tiles_y) return render_impl_band(ctx, scene, sensor, integrator, spp, max_depth, seed, sample_offset, out, out_is_device, stats, nullptr);
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    trhip_stats sum;
    std::memset(&sum, 0, sizeof sum);
    uint32_t n_bands = 0;
    for (int t0 = 0; t0 < ds.tiles_y; t0 += rows_per_band, ++n_bands) {
        const DeviceSensor b = band_of(ds, t0, rows_per_band);
        trhip_stats st;
        if (int rc = render_impl_band(ctx, scene, sensor, integrator, spp, max_depth, seed, sample_offset, d_film, true, &st, &b)) return rc;
        stats_accumulate(sum, st);
    }
    ctx->last = LastRecords{};  // trhip_last_sample_radiance describes whole frames only
    if (int rc = copy_back(ctx, out, out_is_device, d_film, film_bytes)) return rc;
    if (stats) *stats = sum;
    return 0;
}
// trhip_render_path_map[_device]: the refusals that belong to the map, in the header's order, then the job list, then the frame.
int render_map_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, const void* counts, bool on_device, uint32_t max_spp, int max_depth, uint64_t seed, uint32_t sample_offset,
                    void* out, trhip_stats* stats) {
    if (!ctx || !scene || !sensor || !counts || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (max_spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "max_spp must be >= 1");
    DeviceSensor ds;
    derive_sensor(sensor, ds);
    if (ds.film_w <= 0 || ds.film_h <= 0 || ds.sb_w <= 0 || ds.sb_h <= 0) return fail(ctx, TRHIP_ERR_INVALID, "empty film");
    const uint64_t npix = (uint64_t)ds.sb_w * ds.sb_h;
    if (npix >= (1ull << 31) || npix * max_spp >= (1ull << 32)) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "more than 2^32 camera samples at max_spp in a map frame");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t total = 0;
    bool above = false;
    if (on_device) {
        if (ctx->last.kind == 2) ctx->last = LastRecords{};  // the counts of the map frame before go with this copy
        if (int rc = ensure(ctx, ctx->map_counts, npix * sizeof(uint32_t))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->map_counts.p, counts, npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        const uint32_t* c = (const uint32_t*)counts;
        for (uint64_t p = 0; p < npix; ++p) {
            total += c[p];
            above = above || c[p] > max_spp;
        }
        if (!above && total)
            if (int rc = upload(ctx, ctx->map_counts, counts, npix * sizeof(uint32_t))) return rc;
    }
    if (!above && (on_device || total))
        if (int rc = map_job_list(ctx, (uint32_t)npix, max_spp, on_device, &total, &above)) return rc;
    if (above) return fail(ctx, TRHIP_ERR_INVALID, "a count of the sample map lies above max_spp = %u", max_spp);
    if (total == 0) return fail(ctx, TRHIP_ERR_INVALID, "the sample map draws no sample");
    const MapFrame map{(const uint32_t*)ctx->map_counts.p, (const uint32_t*)ctx->map_jobs.p, total};
    ctx->last = LastRecords{};  // (until this frame's radiance is complete: map_counts already belongs to it)
    return render_path_frame(ctx, scene, sensor, max_spp, max_depth, seed, sample_offset, out, on_device, stats, &map, nullptr);
}
}  // namespace

int render_path_frame(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, void* out, bool out_is_device,
                      trhip_stats* stats, const MapFrame* map, PathTerm* term) {
    return render_impl_band(ctx, scene, sensor, 1, spp, max_depth, seed, sample_offset, out, out_is_device, stats, nullptr, map, term);
}

extern "C" {

int trhip_plan_bands(const trhip_sensor* sensor, uint32_t spp, uint64_t budget_bytes, uint32_t bytes_per_sample, uint32_t cap, uint32_t* n_bands, int32_t* first_row, int32_t* n_rows) {
    if (!sensor || !n_bands || spp == 0 || bytes_per_sample == 0) return TRHIP_ERR_INVALID;
    DeviceSensor ds;
    derive_sensor(sensor, ds);
    if (ds.sb_w <= 0 || ds.sb_h <= 0) return TRHIP_ERR_INVALID;
    const int rows = plan_rows_per_band(ds, spp, (double)budget_bytes, (double)bytes_per_sample);
    uint32_t n = 0;
    for (int t0 = 0; t0 < ds.tiles_y; t0 += rows, ++n) {
        const DeviceSensor b = band_of(ds, t0, rows);
        if (n < cap) {
            if (first_row) first_row[n] = b.band_y0;
            if (n_rows) n_rows[n] = b.band_rows;
        }
    }
    *n_bands = n;
    return 0;
}


int trhip_render_path(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, float* out, trhip_stats* st) {
    return render_impl(ctx, sc, sn, 1, spp, max_depth, seed, off, out, false, st);
}
int trhip_render_path_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, void* d_out, trhip_stats* st) {
    return render_impl(ctx, sc, sn, 1, spp, max_depth, seed, off, d_out, true, st);
}
int trhip_render_whitted(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, float* out, trhip_stats* st) {
    return render_impl(ctx, sc, sn, 0, spp, max_depth, seed, off, out, false, st);
}
int trhip_render_whitted_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, void* d_out, trhip_stats* st) {
    return render_impl(ctx, sc, sn, 0, spp, max_depth, seed, off, d_out, true, st);
}
int trhip_render_path_map(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, const uint32_t* counts, uint32_t max_spp, int max_depth, uint64_t seed, uint32_t off, float* out,
                          trhip_stats* st) {
    return render_map_impl(ctx, sc, sn, counts, false, max_spp, max_depth, seed, off, out, st);
}
int trhip_render_path_map_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, const void* d_counts, uint32_t max_spp, int max_depth, uint64_t seed, uint32_t off, void* d_out,
                                 trhip_stats* st) {
    return render_map_impl(ctx, sc, sn, d_counts, true, max_spp, max_depth, seed, off, d_out, st);
}
int trhip_last_sample_radiance(trhip_ctx* ctx, float* out, uint64_t n_floats) {
    if (!ctx || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    const LastRecords& last = ctx->last;
    if (n_floats != last.count * 3) return fail(ctx, TRHIP_ERR_INVALID, "expected %llu floats", (unsigned long long)(last.count * 3));
    return read_back_records(ctx, out, n_floats, [&](void* dst, dim3 grid) {
        if (last.kind == 2)  // a map frame: the records that were drawn, +0 elsewhere
            hipLaunchKernelGGL(k_export_L_map, grid, dim3(256), 0, ctx->stream, (const float4*)ctx->Lbuf.p, last.count, (float*)dst, last.layout, last.npix, last.spp, (const uint32_t*)ctx->map_counts.p);
        else
            hipLaunchKernelGGL(k_export_L, grid, dim3(256), 0, ctx->stream, (const float4*)ctx->Lbuf.p, last.count, (float*)dst, last.layout, last.npix, last.spp);
    });
}
int trhip_film_to_rgb(trhip_ctx* ctx, const float* xyzw, uint32_t w, uint32_t h, float scale, float* out) {
    if (!ctx || !xyzw || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n = w * h;
    if (int rc = upload(ctx, ctx->scratch[0], xyzw, (size_t)n * 4 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], (size_t)n * 3 * sizeof(float))) return rc;
    if (n) hipLaunchKernelGGL(k_film_to_rgb, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)ctx->scratch[0].p, n, scale, (float*)ctx->scratch[1].p);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->scratch[1].p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int trhip_generate_rays(trhip_ctx* ctx, const trhip_sensor* sn, const float* samples5, uint64_t n, float* out8) {
    if (!ctx || !sn || !samples5 || !out8) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceSensor ds;
    derive_sensor(sn, ds);
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->scratch[0], samples5, n * 5 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], n * 8 * sizeof(float))) return rc;
    if (n) hipLaunchKernelGGL(k_generate_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const DeviceSensor*)ctx->sensor.p, (const float*)ctx->scratch[0].p, (uint32_t)n,
                              (float*)ctx->scratch[1].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out8, ctx->scratch[1].p, n * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int trhip_bsdf_query(trhip_ctx* ctx, const trhip_scene* sc, uint32_t material, int multi, int mode, int flags, const float* frame9, const float* dirs6, uint64_t n, float* out8) {
    if (!ctx || !sc || !frame9 || !dirs6 || !out8) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!sc->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    if (material >= sc->g->materials.size()) return fail(ctx, TRHIP_ERR_INVALID, "material %u not defined", material);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = upload(ctx, ctx->scratch[0], frame9, n * 9 * sizeof(float))) return rc;
    if (int rc = upload(ctx, ctx->scratch[1], dirs6, n * 6 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[2], n * 8 * sizeof(float))) return rc;
    if (n) hipLaunchKernelGGL(k_bsdf_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sc->dev, material, multi, mode, flags, (const float*)ctx->scratch[0].p,
                              (const float*)ctx->scratch[1].p, (uint32_t)n, (float*)ctx->scratch[2].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out8, ctx->scratch[2].p, n * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int trhip_film_accumulate(trhip_ctx* ctx, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t sample_offset, const float* sample_L, float* out_xyzw) {
    if (!ctx || !sn || !sample_L || !out_xyzw) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceSensor ds;
    derive_sensor(sn, ds);
    const uint64_t n = (uint64_t)ds.sb_w * ds.sb_h * spp;
    if (int rc = upload(ctx, ctx->sensor, &ds, sizeof ds)) return rc;
    if (int rc = upload(ctx, ctx->table, sn->filter_table, 256 * sizeof(float))) return rc;
    if (int rc = upload(ctx, ctx->scratch[0], sample_L, n * 3 * sizeof(float))) return rc;
    ctx->last = LastRecords{};
    if (int rc = ensure(ctx, ctx->Lbuf, n * sizeof(float4))) return rc;
    const size_t film_bytes = (size_t)ds.film_w * ds.film_h * sizeof(float4);
    if (int rc = ensure(ctx, ctx->film, film_bytes)) return rc;
    if (int rc = ensure_film_samples(ctx, film_packed(ds), n)) return rc;
    if (n) hipLaunchKernelGGL(k_import_L, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float*)ctx->scratch[0].p, n, (float4*)ctx->Lbuf.p);
    launch_film(ctx, ctx->stream, ds, (const DeviceSensor*)ctx->sensor.p, (const float4*)ctx->Lbuf.p, n, spp, seed, sample_offset, (float4*)ctx->film.p, false);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last = LastRecords{n, 0u, (uint32_t)((uint64_t)ds.sb_w * ds.sb_h), spp, 1u};  // (trhip_last_sample_stats reads a caller's records too)
    HIP_TRY(ctx, hipMemcpy(out_xyzw, ctx->film.p, film_bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
