// tu_sky.hip — the sky-lit frame (trhip_render_sky; docs/design/25-sky.md): trhip_render_ao's frame (th_occlusion.h: ray generation, the scene's closest-hit walk, the spawn
// kernel, the scene's any-hit walk in its accumulate mode with a per-ray reach, the film pass) with k_sky_spawn (th_sky.h) in k_ao_spawn's place.
#include "th_occlusion.h"
#include "th_sky.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_sky_params) == 16, "trhip_sky_params layout");
constexpr uint32_t kSkyFlags = TRHIP_SKY_ALBEDO | TRHIP_SKY_HIDE_BACKGROUND;

// The map itself lives in the environment handle; everything else is trhip_render_ao's.
int render_sky_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, const trhip_env* env, const trhip_sky_params* prm,
                    void* out, bool out_is_device, trhip_stats* stats) {
    // the parameter block first, as trhip_render_ao: it is checked before any handle is looked at, and none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->max_distance > 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: max_distance must be > 0 or +Inf");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: scale must be finite and >= 0");
    if (prm->flags & ~kSkyFlags) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: unknown flag bits 0x%x", prm->flags & ~kSkyFlags);
    if (prm->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: reserved must be 0");
    if (spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1");
    if (!ctx || !scene || !sensor || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: null environment");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: the environment belongs to another context");
    if (std::isinf(env->max_texel * prm->scale))  // the contributions in the any-hit queue carry no poison bits: they must be finite
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky: scale %g takes the map's largest texel (%g) to +Inf", (double)prm->scale, (double)env->max_texel);
    return occlusion_frame(ctx, scene, sensor, spp, seed, sample_offset, "trhip_render_sky", out, out_is_device, stats, [&](const OcclusionSpawn& f) {
        hipLaunchKernelGGL(k_sky_spawn, dim3(f.grid), dim3(kBlock), 0, f.st, scene->dev, f.base_colour, f.pq, f.sq, f.tmax, f.cap, f.hits, f.n, prm->max_distance, env->dev(), prm->scale,
                           prm->flags & TRHIP_SKY_ALBEDO, prm->flags & TRHIP_SKY_HIDE_BACKGROUND, f.L, f.ctr);
    });
}

}  // namespace

extern "C" {

int trhip_sky_default_params(trhip_sky_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    out->max_distance = kInf;
    out->scale = 1.0f;
    out->flags = 0u;
    out->reserved = 0u;
    return 0;
}
int trhip_render_sky(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_env* env, const trhip_sky_params* prm, float* out_xyzw,
                     trhip_stats* st) {
    return render_sky_impl(ctx, sc, sn, spp, seed, off, env, prm, out_xyzw, false, st);
}
int trhip_render_sky_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_env* env, const trhip_sky_params* prm,
                            void* d_out_xyzw, trhip_stats* st) {
    return render_sky_impl(ctx, sc, sn, spp, seed, off, env, prm, d_out_xyzw, true, st);
}

}  // extern "C"
