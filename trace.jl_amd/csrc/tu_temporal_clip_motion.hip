// tu_temporal_clip_motion.hip — trhip_temporal_clip_motion: the pass of th_temporal_clip_motion.h on a film, its feature planes, its id plane, the caller's body table and body
// matrices and the previous frame's history.  No scene, no traversal: an image-space pass on the scaffold of th_image_pass.h.
#include "th_host.h"
#include "th_temporal_clip_motion.h"
#include "th_image_pass.h"

#include <cmath>
#include <limits>

namespace {

static_assert(sizeof(trhip_temporal_clip_motion_params) == 96, "trhip_temporal_clip_motion_params layout");
static_assert(offsetof(trhip_temporal_clip_motion_params, base) == 0 && sizeof(trhip_temporal_motion_params) == 80 && offsetof(trhip_temporal_clip_motion_params, clip_gamma) == 80 &&
                  offsetof(trhip_temporal_clip_motion_params, clip_radius) == 84 && offsetof(trhip_temporal_clip_motion_params, clip_max_history) == 88 &&
                  offsetof(trhip_temporal_clip_motion_params, reserved2) == 92,
              "trhip_temporal_clip_motion_params: the motion block, then gamma, radius, clip_max_history, reserved2");

constexpr size_t kCmHostBytesPerPixel = 192;  // the host entry point's copies: film 16, planes 48, history 48, new history 48, the result's film 16, ids 16 (and 4 per primitive, 48 per body)

// trhip_temporal_motion's block checks on base, in its order, then the new fields
int check_params(trhip_ctx* ctx, const trhip_temporal_clip_motion_params* cp) {
    const trhip_temporal_motion_params* p = &cp->base;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p->prev_world_to_pixel[i])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: prev_world_to_pixel[%d] is not finite", i);
    if (!(std::isfinite(p->max_history) && p->max_history >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: max_history must be finite and >= 1");
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: sigma_plane must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: min_coverage must lie in [0, 1]");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: unknown flag bits 0x%x", p->flags);
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: reserved must be 0");
    if (!(cp->clip_gamma >= 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: clip_gamma must be >= 0 (+Inf: no clipping)");  // false for NaN
    if (cp->clip_radius < 1 || cp->clip_radius > 3) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: clip_radius must be 1, 2 or 3, not %u", cp->clip_radius);
    if (!(cp->clip_max_history >= 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: clip_max_history must be >= 0 (+Inf: the history length is never cut)");
    if (cp->reserved2 != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: reserved2 must be 0");
    return 0;
}

int clip_motion_impl(trhip_ctx* ctx, const void* xyzw, const void* planes, const void* history, const void* ids, const void* body_of_prim, const void* bodies, uint32_t width,
                     uint32_t height, const trhip_temporal_clip_motion_params* cp, void* out, void* out_history, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!cp) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, cp)) return rc;
    const trhip_temporal_motion_params* prm = &cp->base;
    if (!ctx || !xyzw || !planes || !out || !out_history) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (!ids && prm->n_prims > 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: ids may be null only with n_prims = 0, not %u", prm->n_prims);
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: empty film (%u x %u)", width, height);
    if (prm->n_prims > 0 && !body_of_prim) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: n_prims = %u but body_of_prim is null", prm->n_prims);
    if (prm->n_bodies > 0 && !bodies) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: n_bodies = %u but bodies is null", prm->n_bodies);
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, ids_bytes = (size_t)npix * sizeof(int4);
    const size_t table_bytes = (size_t)prm->n_prims * sizeof(uint32_t), bodies_bytes = (size_t)prm->n_bodies * 12 * sizeof(float);
    // trhip_temporal's four, then the three arrays this pass reads beside them
    const ByteRange frame[7] = {{xyzw, film_bytes}, {planes, planes_bytes}, {history, planes_bytes}, {out, film_bytes}, {ids, ids_bytes}, {table_bytes ? body_of_prim : nullptr, table_bytes}, {bodies_bytes ? bodies : nullptr, bodies_bytes}};
    if (overlaps_any(out_history, planes_bytes, frame, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: out_history overlaps an input or out_xyzw");
    if (overlaps_any(out, film_bytes, frame + 4, 3)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip_motion: out_xyzw overlaps ids, body_of_prim or bodies");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    // The kernel's staging reads the film pixels of a whole window, so it cannot write the film it reads: the host variant has a film of its own for the result, and a device
    // out_xyzw that is (or overlaps) xyzw is written through a film held by the context and copied (trhip_temporal_clip's way).  The images in the order of the host layout:
    // the 16-byte records first, the table last, so that each keeps its alignment in the staging buffer whatever n_prims is
    ImageStaging images(ctx, ctx->tp_in, is_device);
    const ImageStaging::Image& film = images.input(xyzw, film_bytes);
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
    const ImageStaging::Image& result = images.output_apart(out, film_bytes, film);
    const ImageStaging::Image& id_plane = images.input(ids, ids_bytes);
    const ImageStaging::Image& matrices = images.input(bodies, bodies_bytes);
    const ImageStaging::Image& table = images.input(body_of_prim, table_bytes);
    {
        const size_t held = ctx->tp_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (by > 65535u || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED,
                        "trhip_temporal_clip_motion: the images of a %u x %u film (%.1f GB, %u B per pixel) do not fit in free HBM (%.1f GB free); there are no bands here", width, height,
                        need * 1e-9, (unsigned)kCmHostBytesPerPixel, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const TemporalConst k = temporal_const<TemporalConst>(*prm);
    // an empty array is never read: the kernel sees it as absent (a staged image of zero bytes has an address all the same)
    const uint32_t* d_table = prm->n_prims ? table.in<uint32_t>() : nullptr;
    const float* d_bodies = prm->n_bodies ? matrices.in<float>() : nullptr;
    const int4* d_ids = prm->n_prims ? id_plane.in<int4>() : nullptr;  // without a table every pixel is static before anything is read

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    const dim3 grid(bx, by), block(kDnTile * kDnTile);
#define TRHIP_LAUNCH_CLIP_MOTION(R)                                                                                                                                                    \
    hipLaunchKernelGGL((k_temporal_clip_motion<R>), grid, block, 0, w.st, film.in<float4>(), guides.in<float4>(), old_history.in<float4>(), d_ids, d_table, d_bodies, (int)width, \
                       (int)height, k, cp->clip_gamma, cp->clip_max_history, prm->n_prims, prm->n_bodies, result.out<float4>(), new_history.out<float4>())
    if (cp->clip_radius == 1)
        TRHIP_LAUNCH_CLIP_MOTION(1);
    else if (cp->clip_radius == 2)
        TRHIP_LAUNCH_CLIP_MOTION(2);
    else
        TRHIP_LAUNCH_CLIP_MOTION(3);
#undef TRHIP_LAUNCH_CLIP_MOTION
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

}  // namespace

extern "C" {

int trhip_temporal_clip_motion_default_params(trhip_temporal_clip_motion_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    if (int rc = trhip_temporal_motion_default_params(&out->base)) return rc;
    trhip_temporal_clip_params clip;
    if (int rc = trhip_temporal_clip_default_params(&clip)) return rc;
    out->clip_gamma = clip.clip_gamma;
    out->clip_radius = clip.clip_radius;
    // The rule stated before the sweep ran (docs/design/21-clip-motion.md): among the cells with finite gamma the lowest geometric mean, over the still and the arc sequence,
    // of the whole-frame MSE ratio to the unclipped motion-aware session; ties to the larger clip_max_history.  It picks gamma 4, R 3, +Inf (1.014; 4: 1.015, 2: 1.023,
    // 1: 1.040, 0: 1.130; profiles/r18/clip_motion.txt): at 2 spp cutting the history of a clipped pixel costs more noise than the stale colour it removes.  After a change
    // of lights a finite value pays (0: 0.0134 against 0.0215 in the first frame): a caller whose lighting jumps sets it
    out->clip_max_history = std::numeric_limits<float>::infinity();
    return 0;
}
int trhip_temporal_clip_motion(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim, const float* bodies,
                               uint32_t width, uint32_t height, const trhip_temporal_clip_motion_params* prm, float* out_xyzw, float* out_history, trhip_stats* st) {
    return clip_motion_impl(ctx, xyzw, planes, history, ids, body_of_prim, bodies, width, height, prm, out_xyzw, out_history, false, st);
}
int trhip_temporal_clip_motion_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, const void* d_ids, const void* d_body_of_prim, const void* d_bodies,
                                      uint32_t width, uint32_t height, const trhip_temporal_clip_motion_params* prm, void* d_out_xyzw, void* d_out_history, trhip_stats* st) {
    return clip_motion_impl(ctx, d_xyzw, d_planes, d_history, d_ids, d_body_of_prim, d_bodies, width, height, prm, d_out_xyzw, d_out_history, true, st);
}

}  // extern "C"
