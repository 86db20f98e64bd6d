// tu_path_env.hip — the environment term of path frames (trhip_render_path_env, trhip_last_escapes, trhip_path_env_relight; docs/design/26-path-env.md).  The frame is
// tu_path.hip's classic wavefront, handed a PathEnvFrame; this unit holds the two kernels it launches for it (th_path_env.h) — in a unit of their own, so that tu_path.hip
// instantiates what it instantiated before — the parameter checks, the read-back of the records and the relight.
#include "th_path_env.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_path_env_params) == 16, "trhip_path_env_params layout");
static_assert(TRHIP_PATH_ENV_HIDE_BACKGROUND == kPathEnvHideBackground, "the kernel's flag bit");
constexpr uint32_t kPathEnvFlags = TRHIP_PATH_ENV_HIDE_BACKGROUND;

// the parameter block: checked before any handle is looked at, and none of it needs a device
int check_params(trhip_ctx* ctx, const trhip_path_env_params* prm, const char* entry) {
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "%s: scale must be finite and >= 0", entry);
    if (prm->flags & ~kPathEnvFlags) return fail(ctx, TRHIP_ERR_INVALID, "%s: unknown flag bits 0x%x", entry, prm->flags & ~kPathEnvFlags);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "%s: reserved must be 0", entry);
    return 0;
}

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_env* env,
                const trhip_path_env_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    if (int rc = check_params(ctx, prm, "trhip_render_path_env")) return rc;
    return render_path_env_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, env, prm->scale, prm->flags);
}

// Another environment and / or other parameters over the retained records, then the film pass exactly as the frame ran it (ctx->env_keep).
int relight_impl(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, void* out, bool out_is_device) {
    if (int rc = check_params(ctx, prm, "trhip_path_env_relight")) return rc;
    if (!ctx || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!ctx->last.path_env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_path_env_relight: the context's last frame is not a path-env frame");
    if (ctx->last.path_env == 2)  // (tu_path_nee.hip: the base records hold the map's direct light, which no fold can exchange)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_path_env_relight: the context's last frame was rendered with next-event estimation (trhip_render_path_env_nee): its base radiance contains the map");
    if (int rc = path_env_check(ctx, env, prm->scale)) return rc;
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
    const PathEnvFrame f{env, prm->scale, prm->flags, (float4*)ctx->env_base.p, (float4*)ctx->env_rec.p};
    launch_escape_fold(ctx, st, f, k.l_slots, (float4*)ctx->Lbuf.p);
    launch_film(ctx, st, k.ds, (const DeviceSensor*)ctx->sensor.p, (const float4*)ctx->Lbuf.p, k.total_slots, k.spp, k.seed, k.sample_offset, (float4*)d_film, k.fused);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->last = last;
    return copy_back(ctx, out, out_is_device, d_film, film_bytes);
}

}  // namespace

int path_env_check(trhip_ctx* ctx, const trhip_env* env, float scale) {
    if (!env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: null environment");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: the environment belongs to another context");
    if (std::isinf(env->max_texel * scale))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env: scale %g takes the map's largest texel (%g) to +Inf", (double)scale, (double)env->max_texel);
    return 0;
}
void launch_path_escape(trhip_ctx* ctx, hipStream_t st, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, float4* rec) {
    // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
    hipLaunchKernelGGL(k_path_escape, dim3(grid_for(ctx, (uint64_t)cap * kSeg, 8)), dim3(kBlock), 0, st, counts, cap, q, hits, (uint32_t)depth, rec);
}
void launch_escape_fold(trhip_ctx* ctx, hipStream_t st, const PathEnvFrame& f, uint64_t l_slots, float4* out) {
    hipLaunchKernelGGL(k_escape_fold, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)f.base, (const float4*)f.rec, l_slots, f.env->dev(), f.scale, f.flags, out);
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
    if (!last.path_env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_last_escapes: the context's last frame is not a path-env frame");
    if (n_floats != last.count * 8) return fail(ctx, TRHIP_ERR_INVALID, "expected %llu floats", (unsigned long long)(last.count * 8));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, ctx->scratch[0], n_floats * sizeof(float))) return rc;
    const uint64_t n = last.count;
    if (n) hipLaunchKernelGGL(k_export_escapes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float4*)ctx->env_rec.p, n, (float4*)ctx->scratch[0].p, last.layout, last.npix, last.spp);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out8, ctx->scratch[0].p, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int trhip_path_env_relight(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, float* out_xyzw) { return relight_impl(ctx, env, prm, out_xyzw, false); }
int trhip_path_env_relight_device(trhip_ctx* ctx, const trhip_env* env, const trhip_path_env_params* prm, void* d_out_xyzw) { return relight_impl(ctx, env, prm, d_out_xyzw, true); }

}  // extern "C"
