// tu_ao.hip — ambient occlusion (trhip_render_ao): the path integrator's ray generation and the scene's closest-hit walk, k_ao_spawn (th_ao.h), the scene's any-hit walk in
// its accumulate mode with a per-ray reach, then the path integrator's film pass — the frame of th_occlusion.h, which trhip_render_sky shares.
#include "th_occlusion.h"
#include "th_ao.h"

namespace {

static_assert(sizeof(trhip_ao_params) == 16, "trhip_ao_params layout");

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
    return occlusion_frame(ctx, scene, sensor, spp, seed, sample_offset, "trhip_render_ao", out, out_is_device, stats, [&](const OcclusionSpawn& f) {
        hipLaunchKernelGGL(k_ao_spawn, dim3(f.grid), dim3(kBlock), 0, f.st, scene->dev, f.base_colour, f.pq, f.sq, f.tmax, f.cap, f.hits, f.n, prm->max_distance, prm->background,
                           prm->flags & TRHIP_AO_ALBEDO, f.L, f.ctr);
    });
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
