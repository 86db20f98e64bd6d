// tu_path_nee.hip — next-event estimation of the environment map in path frames (trhip_render_path_env_nee; docs/design/28-path-nee.md).  The frame is tu_path.hip's classic
// wavefront, handed the NEE term: the environment term (th_host.h, EnvTerm) plus the shadow lane.  This unit holds the two kernels the term launches (th_path_nee.h) — in a
// unit of their own, so that tu_path.hip and tu_path_env.hip instantiate what they instantiated before —, the term and the lane (which the emit term shares).
#include "th_path_nee.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_path_nee_params) == 32, "trhip_path_nee_params layout");
static_assert(TRHIP_PATH_ENV_HIDE_BACKGROUND == kPathEnvHideBackground, "the kernel's flag bit");
constexpr uint32_t kPathNeeFlags = TRHIP_PATH_ENV_HIDE_BACKGROUND;
constexpr double kNeeQueueBytes = 2.0 * 3.0 * sizeof(float4);  // per queue entry: two parities of three float4 arrays

struct NeeTerm : EnvTerm {
    float mix, om;  // om = 1 - mix, computed once in Float32: the kernel's (1 - mix)
    NeeTerm(const trhip_env* e, float s, uint32_t f, float m) : EnvTerm(e, s, f), mix(m), om(1.0f - m) {}
    int check(trhip_ctx* ctx, const trhip_scene* scene) override {  // the environment's refusals, then the sampler, then the materials
        if (int rc = EnvTerm::check(ctx, scene)) return rc;
        if (!env->sampler.p) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: the environment has no sampler (trhip_env_make_sampler)");
        return path_mixed_lobes_check(ctx, scene, "trhip_render_path_env_nee");
    }
    double path_bytes() const override { return kNeeQueueBytes; }
    // the path-env frame's per-sample bytes, the note byte and the queues must fit in half of free HBM beside the path-env frame's buffers
    int buffers(trhip_ctx* ctx, const PathTermShape& s) override {
        if (int rc = EnvTerm::buffers(ctx, s)) return rc;
        const size_t held = ctx->Lbuf.bytes + ctx->pfilm.bytes + ctx->env_base.bytes + ctx->env_rec.bytes + ctx->lane.held(false) + held_in_pipes(ctx);
        const double need = (double)s.total_slots * ((65.0 + s.film_bytes) + 1.0) + (double)s.n_pipes * ((double)s.queue_entries * kNeeQueueBytes + (double)sizeof(NeeCounters));
        bool fits = false;
        double free_gb = 0.0;
        if (int rc = fits_in_hbm(ctx, 2.0 * need, held, &fits, &free_gb)) return rc;
        if (!fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "the per-sample buffers and the shadow queues of a path-env frame with next-event estimation (%.2f GB at %u spp) do not fit in half of free HBM (%.2f GB): there are no bands here",
                        need * 1e-9, s.spp, free_gb);
        return ctx->lane.grow(ctx, s.n_pipes, s.queue_entries, s.l_slots, false);
    }
    int clear(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots) override {
        if (int rc = EnvTerm::clear(ctx, st, l_slots)) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->lane.note.p, 0, l_slots, st));  // depth 1 has no vertex before it
        return 0;
    }
    int begin_batch(trhip_ctx* ctx, hipStream_t st, int pipe) override { return ctx->lane.begin_batch(ctx, st, pipe); }
    // k_path_nee stands in k_path_escape's place: the records with their marks, the notes, and the NEE shadow rays of this depth
    void after_closest(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, const uint32_t* counts, uint32_t cap, const PathQueue& q, const float4* hits, int depth, uint32_t hits_have_bary,
                       int pipe) override {
        const size_t lds = (size_t)(env->n + 1u) * sizeof(float);  // the marginal, staged per block: at most 16 KiB (n <= 4096)
        // the queue holds at most kSeg * cap entries; the kernel's grid-stride loop covers whatever the counts say
        hipLaunchKernelGGL(k_path_nee, dim3(grid_for(ctx, (uint64_t)cap * kSeg, 8)), dim3(kBlock), lds, st, scene->dev, counts, cap, q, hits, (uint32_t)depth, hits_have_bary, rec,
                           (uint8_t*)ctx->lane.note.p, env->dev(), env_sampler_dev(env), scale, mix, om, ctx->lane.queue(pipe, depth), ctx->lane.emitted(pipe, depth));
    }
    // the NEE rays directly after the point-light rays: the two terms of one depth reach a slot's record in model order, and no launch holds two writers of one slot
    void after_any(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, int pipe, Counters* ctr, void* overflow_slab) override {
        ctx->lane.launch_any(ctx, st, scene, cap, depth, base, pipe, false, ctr, overflow_slab);
    }
    void fold(trhip_ctx* ctx, hipStream_t st, uint64_t l_slots, float4* out) override {  // k_escape_fold with the suppressed mark
        hipLaunchKernelGGL(k_escape_fold_nee, dim3(grid_for(ctx, l_slots, 8)), dim3(kBlock), 0, st, (const float4*)base, (const float4*)rec, l_slots, env->dev(), scale, flags, out);
    }
    LastRecords::Term kind() const override { return LastRecords::kEnvNee; }
};

int render_impl(trhip_ctx* ctx, const trhip_scene* scene, const trhip_sensor* sensor, uint32_t spp, int max_depth, uint64_t seed, uint32_t sample_offset, const trhip_env* env,
                const trhip_path_nee_params* prm, void* out, bool out_is_device, trhip_stats* stats) {
    if (int rc = path_params_check(ctx, prm, kPathNeeFlags, "trhip_render_path_env_nee")) return rc;
    if (!(prm->mix > 0.0f && prm->mix < 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_render_path_env_nee: mix must lie in (0, 1), not %g", (double)prm->mix);
    NeeTerm term(env, prm->scale, prm->flags, prm->mix);
    return render_path_frame(ctx, scene, sensor, spp, max_depth, seed, sample_offset, out, out_is_device, stats, nullptr, &term);
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

// ---- the shadow lane (th_host.h) ----
size_t ShadowLane::held(bool with_reach) const {
    size_t h = note.bytes;
    for (int pi = 0; pi < kMaxPipes; ++pi)
        for (int k = 0; k < 2; ++k) {
            for (auto& b : sq[pi][k]) h += b.bytes;
            if (with_reach) h += reach[pi][k].bytes;
        }
    return h;
}
int ShadowLane::grow(trhip_ctx* ctx, int n_pipes, uint64_t queue_entries, uint64_t l_slots, bool with_reach) {
    if (int rc = ensure(ctx, note, l_slots)) return rc;
    for (int pi = 0; pi < n_pipes; ++pi) {
        for (int k = 0; k < 2; ++k) {
            for (auto& b : sq[pi][k])
                if (int rc = ensure(ctx, b, queue_entries * sizeof(float4))) return rc;
            if (with_reach)
                if (int rc = ensure(ctx, reach[pi][k], queue_entries * sizeof(float))) return rc;
        }
        if (int rc = ensure(ctx, ctr[pi], sizeof(NeeCounters))) return rc;
    }
    return 0;
}
uint32_t* ShadowLane::emitted(int pipe, int depth) const { return ((NeeCounters*)ctr[pipe].p)->n[depth - 1]; }
int ShadowLane::begin_batch(trhip_ctx* ctx, hipStream_t st, int pipe) {
    HIP_TRY(ctx, hipMemsetAsync(ctr[pipe].p, 0, sizeof(NeeCounters), st));
    return 0;
}
void ShadowLane::launch_any(trhip_ctx* ctx, hipStream_t st, const trhip_scene* scene, uint32_t cap, int depth, float4* L, int pipe, bool with_reach, Counters* c, void* overflow_slab) {
    NeeCounters* nc = (NeeCounters*)ctr[pipe].p;
    const ShadowQueue q = queue(pipe, depth);
    launch_trace(ctx, st, scene, true, SegQueue{nc->n[depth - 1], cap, 0u}, q.o, q.d, with_reach ? (const float*)reach[pipe][depth & 1].p : nullptr, TraceOut{nullptr, L, q.c, nullptr},
                 nc->work[depth - 1], c, overflow_slab);
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
