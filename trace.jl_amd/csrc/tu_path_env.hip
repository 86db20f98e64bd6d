// tu_path_env.hip — the environment term of path frames (trhip_render_path_env, trhip_last_escapes, trhip_path_env_relight; docs/design/26-path-env.md).  The frame is
// tu_path.hip's classic wavefront, handed an EnvTerm (th_host.h); this unit holds the two kernels the term launches (th_path_env.h) — in a unit of their own, so that
// tu_path.hip instantiates what it instantiated before —, the term's hooks, the read-back of the records and the relight.
#include "th_path_env.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_path_env_params) == 16, "trhip_path_env_params layout");
static_assert(TRHIP_PATH_ENV_HIDE_BACKGROUND == kPathEnvHideBackground, "the kernel's flag bit");
constexpr uint32_t kPathEnvFlags = TRHIP_PATH_ENV_HIDE_BACKGROUND;

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_env* env,
                const trhip_path_env_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    if (int rc = path_params_check(ctx, prm, kPathEnvFlags, "trhip_render_path_env")) return rc;
    EnvTerm term(env, prm->scale, prm->flags);
    return render_path_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, nullptr, &term);
}

// Another environment and / or other parameters over the retained records, then the film pass exactly as the frame ran it (ctx->env_keep).
int relight_impl(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, void* out, bool out_is_device) {
    if (int rc = path_params_check(ctx, prm, kPathEnvFlags, "trhip_path_env_relight")) return rc;
    if (!ctx || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!ctx->last.env_records()) return fail(ctx, TRHIP_ERR_INVALID, "trhip_path_env_relight: the context's last frame is not a path-env frame");
    if (ctx->last.term == LastRecords::kEnvNee)  // (tu_path_nee.hip: the base records hold the map's direct light, which no fold can exchange)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_path_env_relight: the context's last frame was rendered with next-event estimation (trhip_render_path_env_nee): its base radiance contains the map");
    EnvTerm term(env, prm->scale, prm->flags);
    if (int rc = term.check(ctx, nullptr)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PathEnvKeep k = ctx->env_keep;
    const LastRecords last = ctx->last;
    if (int rc = upload(ctx, ctx->sensor, &k.ds, sizeof k.ds)) return rc;
    if (int rc = upload(ctx, ctx->table, k.filter_table, sizeof k.filter_table)) return rc;
    if (int rc = ensure_film_samples(ctx, film_packed(k.ds), k.total_slots)) return rc;
    const size_t film_bytes = (size_t)k.ds.film_w * k.ds.film_h * sizeof(float4);
    void* d_film;
    if (int rc = stage_output(ctx, out, out_is_device, film_bytes, &d_film)) return rc;
    ctx->last = LastRecords{};  // (until the fold is complete)
    hipStream_t st = ctx->stream;
    term.base = (float4*)ctx->env_base.p, term.rec = (float4*)ctx->env_rec.p;
    term.fold(ctx, st, k.l_slots, (float4*)ctx->Lbuf.p);
    launch_film(ctx, st, k.ds, (const DeviceSensor*)ctx->sensor.p, (const float4*)ctx->Lbuf.p, k.total_slots, k.spp, k.seed, k.sample_offset, (float4*)d_film, k.fused);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->last = last;
    return copy_back(ctx, out, out_is_device, d_film, film_bytes);
}

}  // namespace

int EnvTerm::check(trhip_ctx* ctx, const trhip_scene*) {
    if (!env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: null environment");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: the environment belongs to another context");
    if (std::isinf(env->max_texel * scale))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: scale %g takes the map's largest texel (%g) to +Inf", (double)scale, (double)env->max_texel);
    return 0;
}
// A path-env frame has no bands: the path's records, their fold, the escape records (16 + 16 + 32 B per slot), the poison byte and what an unfused film pass reads per sample
// must fit in half of what is free, as a map frame's must.
int EnvTerm::early_budget(trhip_ctx* ctx, uint64_t total_slots, double film_bytes, uint32_t spp) {
    bool fits = false;
    double free_gb = 0.0;
    const double need = (double)total_slots * (65.0 + film_bytes);
    const size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->env_base.bytes + ctx->env_rec.bytes + held_in_pipes(ctx);
    if (int rc = fits_in_hbm(ctx, 2.0 * need, held, &fits, &free_gb)) return rc;
    if (!fits) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers of a path-env frame (%.2f GB at %u spp) do not fit in half of free HBM (%.2f GB): there are no bands here", need * 1e-9, spp, free_gb);
    return 0;
}
int EnvTerm::buffers(trhip_ctx* ctx, const PathTermShape& s) {
    if (int rc = ensure(ctx, ctx->env_base, s.l_slots * sizeof(float4))) return rc;
    if (int rc = ensure(ctx, ctx->env_rec, s.l_slots * 2 * sizeof(float4))) return rc;
    base = (float4*)ctx->env_base.p, rec = (float4*)ctx->env_rec.p;
    return 0;
}
int EnvTerm::clear(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots) {
    HIP_TRY(ctx, hipMemsetAsync(rec, 0, l_slots * 2 * sizeof(float4), st));  // depth 0: no escape
    return 0;
}
// every entry that missed leaves its record (one writer per slot; never the base records, which the shadow rays of the depth before may still add to)
void EnvTerm::after_closest(trhip_ctx* ctx, hipStream_t st, const trhip_scene*, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t, int) {
    // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
    hipLaunchKernelGGL(k_path_escape, dim3(grid_for(ctx, (uint64_t)cap * kSeg, 8)), dim3(kBlock), 0, st, counts, cap, q, hits, (uint32_t)depth, rec);
}
// out = base, + beta * (E(dir) * scale) where a record contributes
void EnvTerm::fold(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots, float4* out) {
    hipLaunchKernelGGL(k_escape_fold, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)base, (const float4*)rec, l_slots, env->dev(), scale, flags, out);
}
void EnvTerm::retain(trhip_ctx* ctx, const PathEnvKeep& film_pass) {
    ctx->last.term = kind();
    ctx->env_keep = film_pass;  // what trhip_path_env_relight repeats the film pass with
}

extern "C" {

int trhip_path_env_default_params(trhip_path_env_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    out->scale = 1.0f;
    out->flags = 0u;
    out->reserved[0] = out->reserved[1] = 0u;
    return 0;
}
int trhip_render_path_env(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_env* env,
                          const trhip_path_env_params* prm, float* out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, env, prm, out_xyzw, false, st);
}
int trhip_render_path_env_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_env* env,
                                 const trhip_path_env_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, env, prm, d_out_xyzw, true, st);
}
int trhip_last_escapes(trhip_ctx* ctx, float* out8, uint64_t n_floats) {
    if (!ctx || !out8) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    const LastRecords& last = ctx->last;
    if (!last.env_records()) return fail(ctx, TRHIP_ERR_INVALID, "trhip_last_escapes: the context's last frame is not a path-env frame");
    if (n_floats != last.count * 8) return fail(ctx, TRHIP_ERR_INVALID, "expected %llu floats", (unsigned long long)(last.count * 8));
    return read_back_records(ctx, out8, n_floats, [&](void* dst, dim3 grid) {
        hipLaunchKernelGGL(k_export_escapes, grid, dim3(256), 0, ctx->stream, (const float4*)ctx->env_rec.p, last.count, (float4*)dst, last.layout, last.npix, last.spp);
    });
}
int trhip_path_env_relight(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, float* out_xyzw) { return relight_impl(ctx, env, prm, out_xyzw, false); }
int trhip_path_env_relight_device(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, void* d_out_xyzw) { return relight_impl(ctx, env, prm, d_out_xyzw, true); }

}  // extern "C"
