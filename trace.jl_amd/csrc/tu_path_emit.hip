// tu_path_emit.hip — area lights in path frames (trhip_emitters_*, trhip_render_path_emit, trhip_last_emitted; docs/design/29-path-emit.md).  The frame is tu_path.hip's
// classic wavefront, handed a PathEmitFrame; this unit holds the kernels it launches for it (th_path_emit.h) — in a unit of their own, so that every other unit instantiates
// what it instantiated before —, the emitter set with its table, built here on the host in Float64 in the order the specification gives, the parameter checks, the buffers
// and the launches.
#include "th_path_emit.h"
#include "th_path_nee.h"  // NeeCounters: the emitter shadow queues' counters have their shape

#include <cmath>

static_assert(!std::is_copy_constructible_v<trhip_emitters>, "trhip_emitters (th_path_emit.h) owns its tables: trhip_emitters_free is `delete`");

namespace {

static_assert(sizeof(trhip_path_emit_params) == 32, "trhip_path_emit_params layout");
static_assert(TRHIP_PATH_EMIT_HITS_ONLY == kPathEmitHitsOnly, "the kernel's flag bit");
constexpr uint32_t kPathEmitFlags = TRHIP_PATH_EMIT_HITS_ONLY;
constexpr uint32_t kMaxEmitters = 1u << 20;
constexpr double kEmitQueueBytes = 2.0 * (3.0 * sizeof(float4) + sizeof(float));  // per queue entry: two parities of three float4 arrays and a reach

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_emitters* em,
                const trhip_path_emit_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    // the parameter block: checked before any handle is looked at, and none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: scale must be finite and >= 0");
    if (prm->flags & ~kPathEmitFlags) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: unknown flag bits 0x%x", prm->flags & ~kPathEmitFlags);
    for (int k = 0; k < 6; ++k)
        if (prm->reserved[k] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: reserved must be 0");
    return render_path_emit_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, em, prm->scale, prm->flags);
}

}  // namespace

int path_emit_check(trhip_ctx* ctx, const trhip_scene* scene, const trhip_emitters* em) {
    if (!em) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: null emitters");
    if (em->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: the emitters belong to another context");
    if (em->geometry_id != scene->g->id || em->n_materials != scene->g->materials.size())
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_emit: the emitters were made from another committed geometry (%llu) than the scene's (%llu)", (unsigned long long)em->geometry_id,
                    (unsigned long long)scene->g->id);
    return path_mixed_lobes_check(ctx, scene, "trhip_render_path_emit");
}

int path_emit_buffers(trhip_ctx* ctx, PathEmitFrame& f, int n_pipes, uint64_t queue_entries, uint64_t total_slots, uint64_t l_slots, double film_bytes, uint32_t spp) {
    size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->env_base.bytes + ctx->emit_lh.bytes + ctx->nee_note.bytes + held_in_pipes(ctx);
    for (auto& a : ctx->nee_sq)
        for (auto& b : a)
            for (auto& c : b) held += c.bytes;
    for (auto& a : ctx->emit_tmax)
        for (auto& b : a) held += b.bytes;
    // per slot: the base records, their fold and the emitted sums (16 B each), the poison byte and the note byte; what an unfused film pass reads per sample
    const double need = (double)total_slots * (50.0 + film_bytes) + (double)n_pipes * ((double)queue_entries * kEmitQueueBytes + (double)sizeof(NeeCounters));
    bool fits = false;
    double free_gb = 0.0;
    if (int rc = fits_in_hbm(ctx, 2.0 * need, held, &fits, &free_gb)) return rc;
    if (!fits)
        return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers and the shadow queues of an emit frame (%.2f GB at %u spp) do not fit in half of free HBM (%.2f GB): there are no bands here",
                    need * 1e-9, spp, free_gb);
    if (int rc = ensure(ctx, ctx->env_base, l_slots * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->emit_lh, l_slots * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->nee_note, l_slots)) return rc;
    f.base = (float4*)ctx->env_base.p;
    f.lh = (float4*)ctx->emit_lh.p;
    f.note = (uint8_t*)ctx->nee_note.p;
    for (int pi = 0; pi < n_pipes; ++pi) {
        for (int k = 0; k < 2; ++k) {
            for (int j = 0; j < 3; ++j)
                if (int rc = ensure(ctx, ctx->nee_sq[pi][k][j], queue_entries * sizeof(float4))) return rc;
            if (int rc = ensure(ctx, ctx->emit_tmax[pi][k], queue_entries * sizeof(float))) return rc;
            f.sq[pi][k] = ShadowQueue{(float4*)ctx->nee_sq[pi][k][0].p, (float4*)ctx->nee_sq[pi][k][1].p, (float4*)ctx->nee_sq[pi][k][2].p};
            f.tmax[pi][k] = (float*)ctx->emit_tmax[pi][k].p;
        }
        if (int rc = ensure(ctx, ctx->nee_ctr[pi], sizeof(NeeCounters))) return rc;
        f.ctr[pi] = ctx->nee_ctr[pi].p;
    }
    return 0;
}
void path_emit_begin_batch(trhip_ctx*, hipStream_t st, const PathEmitFrame& f, int pipe) { (void)hipMemsetAsync(f.ctr[pipe], 0, sizeof(NeeCounters), st); }
void launch_path_emit(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t hits_have_bary,
                      const PathEmitFrame& f, int pipe) {
    const trhip_emitters* em = f.em;
    const size_t cdf_bytes = (size_t)(em->n + 1u) * sizeof(float);
    NeeCounters* nc = (NeeCounters*)f.ctr[pipe];
    const dim3 grid(grid_for(ctx, (uint64_t)cap * kSeg, 8));  // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
    if (cdf_bytes <= kEmitCdfLdsBytes)
        hipLaunchKernelGGL(k_path_emit<true>, grid, dim3(kBlock), cdf_bytes, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, f.lh, f.note, em->dev(), f.scale, f.flags,
                           f.sq[pipe][depth & 1], f.tmax[pipe][depth & 1], nc->n[depth - 1]);
    else
        hipLaunchKernelGGL(k_path_emit<false>, grid, dim3(kBlock), 0, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, f.lh, f.note, em->dev(), f.scale, f.flags,
                           f.sq[pipe][depth & 1], f.tmax[pipe][depth & 1], nc->n[depth - 1]);
}
void launch_emit_shadow(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, float4* L, const PathEmitFrame& f, int pipe, Counters* ctr, void* overflow_slab) {
    NeeCounters* nc = (NeeCounters*)f.ctr[pipe];
    const ShadowQueue& sq = f.sq[pipe][depth & 1];
    launch_trace(ctx, st, scene, true, SegQueue{nc->n[depth - 1], cap, 0u}, sq.o, sq.d, f.tmax[pipe][depth & 1], TraceOut{nullptr, L, sq.c, nullptr}, nc->work[depth - 1], ctr, overflow_slab);
}
void launch_emit_fold(trhip_ctx* ctx, hipStream_t st, const PathEmitFrame& f, uint64_t l_slots, float4* out) {
    hipLaunchKernelGGL(k_emit_fold, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)f.base, (const float4*)f.lh, l_slots, out);
}

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
    if (!last.emit) return fail(ctx, TRHIP_ERR_INVALID, "trhip_last_emitted: the context's last frame is not an emit frame");
    if (n_floats != last.count * 4) return fail(ctx, TRHIP_ERR_INVALID, "expected %llu floats", (unsigned long long)(last.count * 4));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, ctx->scratch[0], n_floats * sizeof(float))) return rc;
    const uint64_t n = last.count;
    if (n) hipLaunchKernelGGL(k_export_emitted, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float4*)ctx->emit_lh.p, n, (float4*)ctx->scratch[0].p, last.layout, last.npix, last.spp);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out4, ctx->scratch[0].p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
