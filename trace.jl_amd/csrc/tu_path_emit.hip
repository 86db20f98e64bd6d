// tu_path_emit.hip — area lights in path frames (trhip_emitters_*, trhip_render_path_emit, trhip_last_emitted; docs/design/29-path-emit.md).  The frame is tu_path.hip's
// classic wavefront, handed the emit term (th_host.h, PathTerm); this unit holds the kernels the term launches (th_path_emit.h) — in a unit of their own, so that every other
// unit instantiates what it instantiated before —, the emitter set with its table, built here on the host in Float64 in the order the specification gives, and the term.
#include "th_path_emit.h"
#include "th_path_nee.h"  // NeeCounters: the lane's counters (th_host.h, ShadowLane)

#include <cmath>

static_assert(!std::is_copy_constructible_v<trhip_emitters>, "trhip_emitters (th_path_emit.h) owns its tables: trhip_emitters_free is `delete`");

namespace {

static_assert(sizeof(trhip_path_emit_params) == 32, "trhip_path_emit_params layout");
static_assert(TRHIP_PATH_EMIT_HITS_ONLY == kPathEmitHitsOnly, "the kernel's flag bit");
constexpr uint32_t kPathEmitFlags = TRHIP_PATH_EMIT_HITS_ONLY;
constexpr uint32_t kMaxEmitters = 1u << 20;
constexpr double kEmitQueueBytes = 2.0 * (3.0 * sizeof(float4) + sizeof(float));  // per queue entry: two parities of three float4 arrays and a reach

struct EmitTerm : PathTerm {
    const trhip_emitters* em;
    float scale;
    uint32_t flags;
    float4* lh = nullptr;  // l_slots: {Lh.rgb, counted hits}
    EmitTerm(const trhip_emitters* e, float s, uint32_t f) : em(e), scale(s), flags(f) {}
    int check(trhip_ctx* ctx, const trhip_scene* scene) override {  // null / another context's; another geometry's; a material that mixes lobes
        if (!em) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: null emitters");
        if (em->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: the emitters belong to another context");
        if (em->geometry_id != scene->g->id || em->n_materials != scene->g->materials.size())
            return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: the emitters were made from another committed geometry (%llu) than the scene's (%llu)", (unsigned long long)em->geometry_id,
                        (unsigned long long)scene->g->id);
        return path_mixed_lobes_check(ctx, scene, "trhip_render_path_emit");
    }
    double slot_bytes() const override { return 2.0 * sizeof(float4); }  // the base records and the emitted sums beside Lbuf
    double path_bytes() const override { return kEmitQueueBytes; }
    // the per-sample buffers and the queues must fit in half of free HBM
    int buffers(trhip_ctx* ctx, const PathTermShape& s) override {
        const size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->env_base.bytes + ctx->emit_lh.bytes + ctx->lane.held(true) + held_in_pipes(ctx);
        // per slot: the base records, their fold and the emitted sums (16 B each), the poison byte and the note byte; what an unfused film pass reads per sample
        const double need = (double)s.total_slots * (50.0 + s.film_bytes) + (double)s.n_pipes * ((double)s.queue_entries * kEmitQueueBytes + (double)sizeof(NeeCounters));
        bool fits = false;
        double free_gb = 0.0;
        if (int rc = fits_in_hbm(ctx, 2.0 * need, held, &fits, &free_gb)) return rc;
        if (!fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers and the shadow queues of an emit frame (%.2f GB at %u spp) do not fit in half of free HBM (%.2f GB): there are no bands here",
                        need * 1e-9, s.spp, free_gb);
        if (int rc = ensure(ctx, ctx->env_base, s.l_slots * sizeof(float4))) return rc;
        if (int rc = ensure(ctx, ctx->emit_lh, s.l_slots * sizeof(float4))) return rc;
        base = (float4*)ctx->env_base.p, lh = (float4*)ctx->emit_lh.p;
        return ctx->lane.grow(ctx, s.n_pipes, s.queue_entries, s.l_slots, true);
    }
    int clear(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots) override {
        HIP_TRY(ctx, hipMemsetAsync(ctx->lane.note.p, 0, l_slots, st));  // (depth 1 counts whatever the note says)
        HIP_TRY(ctx, hipMemsetAsync(lh, 0, l_slots * sizeof(float4), st));  // Lh starts at +0
        return 0;
    }
    int begin_batch(trhip_ctx* ctx, hipStream_t st, int pipe) override { return ctx->lane.begin_batch(ctx, st, pipe); }
    // the emitted terms, the notes, and the emitter shadow rays of this depth
    void after_closest(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t hits_have_bary,
                       int pipe) override {
        const ShadowLane& lane = ctx->lane;
        const size_t cdf_bytes = (size_t)(em->n + 1u) * sizeof(float);
        const dim3 grid(grid_for(ctx, (uint64_t)cap * kSeg, 8));  // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
        if (cdf_bytes <= kEmitCdfLdsBytes)
            hipLaunchKernelGGL(k_path_emit<true>, grid, dim3(kBlock), cdf_bytes, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, lh, (uint8_t*)lane.note.p, em->dev(), scale,
                               flags, lane.queue(pipe, depth), (float*)lane.reach[pipe][depth & 1].p, lane.emitted(pipe, depth));
        else
            hipLaunchKernelGGL(k_path_emit<false>, grid, dim3(kBlock), 0, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, lh, (uint8_t*)lane.note.p, em->dev(), scale, flags,
                               lane.queue(pipe, depth), (float*)lane.reach[pipe][depth & 1].p, lane.emitted(pipe, depth));
    }
    // the emitter rays directly after the point-light rays, each with its reach (the NEE term's argument holds: model order, one writer of a slot per launch)
    void after_any(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, int pipe, Counters* ctr, void* overflow_slab) override {
        if (!(flags & TRHIP_PATH_EMIT_HITS_ONLY)) ctx->lane.launch_any(ctx, st, scene, cap, depth, base, pipe, true, ctr, overflow_slab);
    }
    void fold(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots, float4* out) override {  // out = base + Lh
        hipLaunchKernelGGL(k_emit_fold, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)base, (const float4*)lh, l_slots, out);
    }
    void retain(trhip_ctx* ctx, const PathEnvKeep&) override { ctx->last.term = LastRecords::kEmit; }
};

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_emitters* em,
                const trhip_path_emit_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    if (int rc = path_params_check(ctx, prm, kPathEmitFlags, "trhip_render_path_emit")) return rc;
    EmitTerm term(em, prm->scale, prm->flags);
    return render_path_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, nullptr, &term);
}

}  // namespace

extern "C" {

int trhip_emitters_create(trhip_ctx* ctx, const trhip_scene* scene, const uint32_t* material_ids, const float* radiance_rgb3, uint32_t n_materials, trhip_emitters** out) {
    if (!ctx || !scene || !material_ids || !radiance_rgb3 || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (n_materials == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: n_materials must be >= 1");
    for (uint32_t k = 0; k < 3u * n_materials; ++k)
        if (!(radiance_rgb3[k] >= 0.0f) || std::isinf(radiance_rgb3[k]))
            return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: the radiance of material entry %u must be finite and >= 0", k / 3u);
    if (!scene->committed) return fail(ctx, TRHIP_ERR_INVALID, "scene not committed");
    if (scene->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: the scene belongs to another context");
    const SceneGeometry& g = *scene->g;
    const size_t n_mat = g.materials.size();
    std::vector<float4> mat_le(std::max<size_t>(n_mat, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    std::vector<uint8_t> listed(n_mat, 0);
    for (uint32_t k = 0; k < n_materials; ++k) {
        const uint32_t id = material_ids[k];
        if (id >= n_mat) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: material %u not defined", id);
        if (listed[id]) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: material %u is listed twice", id);
        listed[id] = 1;
        mat_le[id] = make_float4(radiance_rgb3[3 * k], radiance_rgb3[3 * k + 1], radiance_rgb3[3 * k + 2], 0.0f);
    }
    for (const HostPrim& p : g.prims)
        if (p.kind == 1 && (p.meta & PRIM_MATERIAL_MASK) < n_mat && listed[p.meta & PRIM_MATERIAL_MASK])
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_emitters_create: material %u is carried by a sphere: only triangles emit", p.meta & PRIM_MATERIAL_MASK);
    // the table, in Float64 from the Float32 world vertices the scene holds, emitters in ascending canonical slot; every sum in the order written
    std::vector<float4> tri;
    std::vector<double> w, a64;
    const uint32_t n_slots = (uint32_t)g.bvh.order.size();
    for (uint32_t slot = 0; slot < n_slots; ++slot) {
        const HostPrim& p = g.prims[g.bvh.order[slot]];
        const uint32_t mat = p.meta & PRIM_MATERIAL_MASK;
        if (p.kind != 0 || mat >= n_mat || !listed[mat]) continue;
        const double e1x = (double)p.v[3] - (double)p.v[0], e1y = (double)p.v[4] - (double)p.v[1], e1z = (double)p.v[5] - (double)p.v[2];
        const double e2x = (double)p.v[6] - (double)p.v[0], e2y = (double)p.v[7] - (double)p.v[1], e2z = (double)p.v[8] - (double)p.v[2];
        const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const double area = 0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz);
        const float4 le = mat_le[mat];
        a64.push_back(area);
        w.push_back(area * (((double)le.x + (double)le.y) + (double)le.z));
        tri.push_back(make_float4(p.v[0], p.v[1], p.v[2], 0.0f));
        tri.push_back(make_float4(p.v[3], p.v[4], p.v[5], 0.0f));
        tri.push_back(make_float4(p.v[6], p.v[7], p.v[8], __builtin_bit_cast(float, slot)));
        tri.push_back(le);
    }
    const size_t n = w.size();
    double total = 0.0;
    for (size_t j = 0; j < n; ++j) total += w[j];
    if (!(total > 0.0)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_create: no triangle of the listed materials has a positive area times radiance: there is nothing to sample");
    if (n > kMaxEmitters) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_emitters_create: %zu emissive triangles, at most %u", n, kMaxEmitters);
    std::vector<float> cdf(n + 1);
    double acc = 0.0;
    for (size_t j = 0; j < n; ++j) {
        cdf[j] = (float)(acc / total);
        acc += w[j];
    }
    cdf[n] = 1.0f;
    for (size_t j = 0; j < n; ++j) {
        tri[4 * j].w = cdf[j + 1] - cdf[j];  // P_j, in Float32
        tri[4 * j + 1].w = (float)a64[j];    // A_j
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<trhip_emitters> em(new trhip_emitters);
    em->ctx = ctx;
    em->geometry_id = g.id;
    em->n = (uint32_t)n;
    em->n_materials = (uint32_t)n_mat;
    if (int rc = upload(ctx, em->tri, tri.data(), tri.size() * sizeof(float4))) return rc;
    if (int rc = upload(ctx, em->cdf, cdf.data(), cdf.size() * sizeof(float))) return rc;
    if (int rc = upload(ctx, em->mat_le, mat_le.data(), mat_le.size() * sizeof(float4))) return rc;
    *out = em.release();
    return 0;
}

void trhip_emitters_free(trhip_emitters* em) {
    if (!em) return;
    (void)hipSetDevice(em->ctx->device);
    delete em;
}

int trhip_emitters_size(const trhip_emitters* em, uint32_t* n_triangles) {
    if (!em || !n_triangles) return TRHIP_ERR_INVALID;
    *n_triangles = em->n;
    return 0;
}

int trhip_emitters_sample(trhip_ctx* ctx, const trhip_emitters* em, const float* u3, uint64_t count, uint32_t* out_index, float* out_point3, float* out_pdf_area) {
    if (!ctx || !em || !u3 || !out_index || !out_point3 || !out_pdf_area) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (em->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_emitters_sample: the emitters belong to another context");
    if (count >= (1ull << 31)) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_emitters_sample: at most 2^31 - 1 entries per call");
    if (count == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = upload(ctx, ctx->scratch[0], u3, (size_t)count * 3 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], (size_t)count * 3 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[2], (size_t)count * sizeof(uint32_t))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[3], (size_t)count * sizeof(float))) return rc;
    hipLaunchKernelGGL(k_emitters_sample, dim3(grid_for(ctx, count, 4)), dim3(kBlock), 0, ctx->stream, em->dev(), (const float*)ctx->scratch[0].p, count, (uint32_t*)ctx->scratch[2].p,
                       (float*)ctx->scratch[1].p, (float*)ctx->scratch[3].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out_point3, ctx->scratch[1].p, (size_t)count * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_index, ctx->scratch[2].p, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_pdf_area, ctx->scratch[3].p, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int trhip_path_emit_default_params(trhip_path_emit_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    *out = trhip_path_emit_params{};
    out->scale = 1.0f;
    return 0;
}
int trhip_render_path_emit(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_emitters* em,
                           const trhip_path_emit_params* prm, float* out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, em, prm, out_xyzw, false, st);
}
int trhip_render_path_emit_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_emitters* em,
                                  const trhip_path_emit_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, em, prm, d_out_xyzw, true, st);
}
int trhip_last_emitted(trhip_ctx* ctx, float* out4, uint64_t n_floats) {
    if (!ctx || !out4) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    const LastRecords& last = ctx->last;
    if (last.term != LastRecords::kEmit) return fail(ctx, TRHIP_ERR_INVALID, "trhip_last_emitted: the context's last frame is not an emit frame");
    if (n_floats != last.count * 4) return fail(ctx, TRHIP_ERR_INVALID, "expected %llu floats", (unsigned long long)(last.count * 4));
    return read_back_records(ctx, out4, n_floats, [&](void* dst, dim3 grid) {
        hipLaunchKernelGGL(k_export_emitted, grid, dim3(256), 0, ctx->stream, (const float4*)ctx->emit_lh.p, last.count, (float4*)dst, last.layout, last.npix, last.spp);
    });
}

}  // extern "C"
