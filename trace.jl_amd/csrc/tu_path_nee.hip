// tu_path_nee.hip — next-event estimation of the environment map in path frames (trhip_render_path_env_nee; docs/design/28-path-nee.md).  The frame is tu_path.hip's classic
// wavefront, handed a PathEnvFrame and a PathNeeFrame; this unit holds the two kernels it launches for it (th_path_nee.h) — in a unit of their own, so that tu_path.hip and
// tu_path_env.hip instantiate what they instantiated before —, the parameter checks, the buffers and the launches.
#include "th_path_nee.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_path_nee_params) == 32, "trhip_path_nee_params layout");
static_assert(TRHIP_PATH_ENV_HIDE_BACKGROUND == kPathEnvHideBackground, "the kernel's flag bit");
constexpr uint32_t kPathNeeFlags = TRHIP_PATH_ENV_HIDE_BACKGROUND;
constexpr double kNeeQueueBytes = 2.0 * 3.0 * sizeof(float4);  // per queue entry: two parities of three float4 arrays

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_env* env,
                const trhip_path_nee_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    // the parameter block: checked before any handle is looked at, and none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!(prm->scale >= 0.0f) || std::isinf(prm->scale)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: scale must be finite and >= 0");
    if (prm->flags & ~kPathNeeFlags) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: unknown flag bits 0x%x", prm->flags & ~kPathNeeFlags);
    for (int k = 0; k < 5; ++k)
        if (prm->reserved[k] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: reserved must be 0");
    if (!(prm->mix > 0.0f && prm->mix < 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: mix must lie in (0, 1), not %g", (double)prm->mix);
    return render_path_env_nee_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, env, prm->scale, prm->flags, prm->mix);
}

}  // namespace

int path_mixed_lobes_check(trhip_ctx* ctx, const trhip_scene* scene, const char* entry) {
    // A lobe set with specular AND non-specular lobes: the vertex would be "non-specular", what follows it suppressed, and the specular lobe's share of the light lost.
    // trhip_scene_add_material builds no such set; checked over the materials, on the host.
    constexpr int NS = BSDF_ALL & ~BSDF_SPECULAR;
    const std::vector<MaterialRec>& mats = scene->g->materials;
    for (size_t m = 0; m < mats.size(); ++m) {
        const LobeSet& b = mats[m].set[1];  // compute_scattering!(si, ray, true): the set a path frame shades with
        int n_ns = 0;
        for (int k = 0; k < b.n; ++k) n_ns += (b.lobe[k].type & NS) == b.lobe[k].type ? 1 : 0;
        if (n_ns != 0 && n_ns != b.n)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "%s: material %zu mixes specular and non-specular lobes: next-event estimation would be biased", entry, m);
    }
    return 0;
}
int path_nee_check(trhip_ctx* ctx, const trhip_scene* scene, const trhip_env* env) {
    if (!env->sampler.p) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: the environment has no sampler (trhip_env_make_sampler)");
    return path_mixed_lobes_check(ctx, scene, "trhip_render_path_env_nee");
}

int path_nee_buffers(trhip_ctx* ctx, PathNeeFrame& f, int n_pipes, uint64_t queue_entries, uint64_t total_slots, uint64_t l_slots, double sample_bytes, uint32_t spp) {
    size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->env_base.bytes + ctx->env_rec.bytes + ctx->nee_note.bytes + held_in_pipes(ctx);
    for (auto& a : ctx->nee_sq)
        for (auto& b : a)
            for (auto& c : b) held += c.bytes;
    const double need = (double)total_slots * (sample_bytes + 1.0) + (double)n_pipes * ((double)queue_entries * kNeeQueueBytes + (double)sizeof(NeeCounters));
    bool fits = false;
    double free_gb = 0.0;
    if (int rc = fits_in_hbm(ctx, 2.0 * need, held, &fits, &free_gb)) return rc;
    if (!fits)
        return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers and the shadow queues of a path-env frame with next-event estimation (%.2f GB at %u spp) do not fit in half of free HBM (%.2f GB): there are no bands here",
                    need * 1e-9, spp, free_gb);
    if (int rc = ensure(ctx, ctx->nee_note, l_slots)) return rc;
    f.note = (uint8_t*)ctx->nee_note.p;
    for (int pi = 0; pi < n_pipes; ++pi) {
        for (int k = 0; k < 2; ++k) {
            for (int j = 0; j < 3; ++j)
                if (int rc = ensure(ctx, ctx->nee_sq[pi][k][j], queue_entries * sizeof(float4))) return rc;
            f.sq[pi][k] = ShadowQueue{(float4*)ctx->nee_sq[pi][k][0].p, (float4*)ctx->nee_sq[pi][k][1].p, (float4*)ctx->nee_sq[pi][k][2].p};
        }
        if (int rc = ensure(ctx, ctx->nee_ctr[pi], sizeof(NeeCounters))) return rc;
        f.ctr[pi] = ctx->nee_ctr[pi].p;
    }
    return 0;
}
void path_nee_begin_batch(trhip_ctx*, hipStream_t st, const PathNeeFrame& f, int pipe) { (void)hipMemsetAsync(f.ctr[pipe], 0, sizeof(NeeCounters), st); }
void launch_path_nee(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t hits_have_bary,
                     const PathEnvFrame& ef, const PathNeeFrame& f, int pipe) {
    const trhip_env* env = ef.env;
    const size_t lds = (size_t)(env->n + 1u) * sizeof(float);  // the marginal, staged per block: at most 16 KiB (n <= 4096)
    NeeCounters* nc = (NeeCounters*)f.ctr[pipe];
    // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
    hipLaunchKernelGGL(k_path_nee, dim3(grid_for(ctx, (uint64_t)cap * kSeg, 8)), dim3(kBlock), lds, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, ef.rec, f.note, env->dev(),
                       env_sampler_dev(env), ef.scale, f.mix, f.om, f.sq[pipe][depth & 1], nc->n[depth - 1]);
}
void launch_nee_shadow(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, float4* L, const PathNeeFrame& f, int pipe, Counters* ctr, void* overflow_slab) {
    NeeCounters* nc = (NeeCounters*)f.ctr[pipe];
    const ShadowQueue& sq = f.sq[pipe][depth & 1];
    launch_trace(ctx, st, scene, true, SegQueue{nc->n[depth - 1], cap, 0u}, sq.o, sq.d, nullptr, TraceOut{nullptr, L, sq.c, nullptr}, nc->work[depth - 1], ctr, overflow_slab);
}
void launch_escape_fold_nee(trhip_ctx* ctx, hipStream_t st, const PathEnvFrame& f, uint64_t l_slots, float4* out) {
    hipLaunchKernelGGL(k_escape_fold_nee, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)f.base, (const float4*)f.rec, l_slots, f.env->dev(), f.scale, f.flags, out);
}

extern "C" {

int trhip_path_nee_default_params(trhip_path_nee_params* out) {
    if (!out) return TRHIP_ERR_INVALID;
    *out = trhip_path_nee_params{};
    out->scale = 1.0f;
    out->mix = 0.5f;
    return 0;
}
int trhip_render_path_env_nee(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_env* env,
                              const trhip_path_nee_params* prm, float* out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, env, prm, out_xyzw, false, st);
}
int trhip_render_path_env_nee_device(trhip_ctx* ctx, const trhip_scene* sc, const trhip_sensor* sn, uint32_t spp, int max_depth, uint64_t seed, uint32_t off, const trhip_env* env,
                                     const trhip_path_nee_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return render_impl(ctx, sc, sn, spp, max_depth, seed, off, env, prm, d_out_xyzw, true, st);
}

}  // extern "C"
