// tu_sky_is.hip — the importance-sampled sky frame (trhip_render_sky_is; docs/design/27-sky-importance.md): trhip_render_sky's frame (th_occlusion.h) with k_sky_spawn_is
// (th_sky_is.h) in k_sky_spawn's place.
#include "th_occlusion.h"
#include "th_sky_is.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_sky_is_params) == 32, "trhip_sky_is_params layout");
constexpr uint32_t kSkyIsFlags = TRHIP_SKY_ALBEDO | TRHIP_SKY_HIDE_BACKGROUND;

int render_sky_is_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, uint64_t seed, uint32_t sample_offset, const trhip_env* env,
                       const trhip_sky_is_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    // the parameter block first, as trhip_render_sky, in its order; then mix, which needs no device either
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->max_distance > 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: max_distance must be > 0 or +Inf");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: scale must be finite and >= 0");
    if (prm->flags & ~kSkyIsFlags) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: unknown flag bits 0x%x", prm->flags & ~kSkyIsFlags);
    for (int k = 0; k < 4; ++k)
        if (prm->reserved[k] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: reserved must be 0");
    if (!(prm->mix > 0.0f && prm->mix < 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: mix must lie in (0, 1), not %g", (double)prm->mix);
    if (spp == 0) return fail(ctx, TRHIP_ERR_INVALID, "spp must be >= 1");
    if (!ctx || !scene || !sensor || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!env) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: null environment");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: the environment belongs to another context");
    if (std::isinf(env->max_texel * prm->scale))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: scale %g takes the map's largest texel (%g) to +Inf", (double)prm->scale, (double)env->max_texel);
    if (!env->sampler.p) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: the environment has no sampler (trhip_env_make_sampler)");
    const float om = 1.0f - prm->mix;  // once, in Float32: the kernel's (1 - mix)
    // a contribution is E * scale * g with g <= 1 / (1 - mix); the any-hit queue carries no poison bits, so that bound must be finite
    if (!(om > 0.0f) || std::isinf((env->max_texel * prm->scale) / om))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_sky_is: scale %g over 1 - mix = %g takes the map's largest texel (%g) to +Inf", (double)prm->scale, (double)om, (double)env->max_texel);
    return occlusion_frame(ctx, scene, sensor, spp, seed, sample_offset, "trhip_render_sky_is", out, out_is_device, stats, [&](const OcclusionSpawn& f) {
        const size_t lds = (size_t)(env->n + 1u) * sizeof(float);  // the marginal, staged per block: at most 16 KiB (n <= 4096)
        hipLaunchKernelGGL(k_sky_spawn_is, dim3(f.grid), dim3(kBlock), lds, f.st, scene->dev, f.base_colour, f.pq, f.sq, f.tmax, f.cap, f.hits, f.n, prm->max_distance, env->dev(),
                           env_sampler_dev(env), prm->scale, prm->mix, om, prm->flags & TRHIP_SKY_ALBEDO, prm->flags & TRHIP_SKY_HIDE_BACKGROUND, f.L, f.ctr);
    });
}

}  // namespace

extern "C" {

int trhip_sky_is_default_params(trhip_sky_is_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    *out = trhip_sky_is_params{};
    out->max_distance = kInf;
    out->scale = 1.0f;
    out->mix = 0.5f;
    return 0;
}
int trhip_render_sky_is(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_env* env, const trhip_sky_is_params* prm,
                        float* out_xyzw, trhip_stats* st) {
    return render_sky_is_impl(ctx, sc, sn, spp, seed, off, env, prm, out_xyzw, false, st);
}
int trhip_render_sky_is_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, uint64_t seed, uint32_t off, const trhip_env* env,
                               const trhip_sky_is_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return render_sky_is_impl(ctx, sc, sn, spp, seed, off, env, prm, d_out_xyzw, true, st);
}

}  // extern "C"
