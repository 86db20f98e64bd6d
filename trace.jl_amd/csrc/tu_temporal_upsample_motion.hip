// tu_temporal_upsample_motion.hip — trhip_temporal_upsample_motion: the pass of th_temporal_upsample_motion.h on a jittered low-resolution film and its planes, the planes and
// the id plane of the full-size sensor, the caller's body table and body matrices and the previous frame's full-size history.  No scene, no traversal: an image-space pass on
// the scaffold of th_image_pass.h.
#include "th_host.h"
#include "th_temporal_upsample_motion.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_temporal_upsample_motion_params) == 128, "trhip_temporal_upsample_motion_params layout");
static_assert(offsetof(trhip_temporal_upsample_motion_params, base) == 0 && sizeof(trhip_temporal_upsample_params) == 112 && offsetof(trhip_temporal_upsample_motion_params, n_prims) == 112 &&
                  offsetof(trhip_temporal_upsample_motion_params, n_bodies) == 116 && offsetof(trhip_temporal_upsample_motion_params, motion_flags) == 120 &&
                  offsetof(trhip_temporal_upsample_motion_params, reserved2) == 124,
              "trhip_temporal_upsample_motion_params: the upsampling block, then n_prims, n_bodies, motion_flags, reserved2");

// trhip_temporal_upsample's block checks on base, in its order, then the new fields
int check_params(trhip_ctx* ctx, const trhip_temporal_upsample_motion_params* mp) {
    const trhip_temporal_upsample_params* p = &mp->base;
    if (int rc = check_lo_from_hi(ctx, "trhip_temporal_upsample_motion", p->lo_from_hi)) return rc;
    if (p->radius != 1 && p->radius != 2) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: radius must be 1 or 2, not %u", p->radius);
    if (!positive_finite(p->guide_sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: guide_sigma_normal must be finite and > 0");
    if (!positive_finite(p->guide_sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: guide_sigma_plane must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: min_coverage must lie in [0, 1]");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: unknown flag bits 0x%x (demodulation and coverage are not offered here)", p->flags);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: reserved must be 0");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p->prev_world_to_pixel[i])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: prev_world_to_pixel[%d] is not finite", i);
    if (!(std::isfinite(p->max_history) && p->max_history >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: max_history must be finite and >= 1");
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: sigma_plane must be finite and > 0");
    if (!(p->confidence_floor > 0.0f && p->confidence_floor <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: confidence_floor must lie in (0, 1]");
    if (!(p->confidence_sharpness >= 0.0f && p->confidence_sharpness <= 4.0f))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: confidence_sharpness must lie in [0, 4]");
    if (mp->motion_flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: unknown motion_flags bits 0x%x", mp->motion_flags);
    if (mp->reserved2 != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: reserved2 must be 0");
    return 0;
}

int impl(trhip_ctx* ctx, const void* lo_xyzw, const void* lo_planes, uint32_t lo_width, uint32_t lo_height, const void* hi_planes, const void* history, const void* ids,
         const void* body_of_prim, const void* bodies, uint32_t width, uint32_t height, const trhip_temporal_upsample_motion_params* mp, void* out, void* out_history, void* out_mask,
         bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!mp) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, mp)) return rc;
    const trhip_temporal_upsample_params* prm = &mp->base;
    if (!ctx || !lo_xyzw || !lo_planes || !hi_planes || !out || !out_history) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0 || lo_width == 0 || lo_height == 0)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: empty image (%u x %u from %u x %u)", width, height, lo_width, lo_height);
    const uint64_t npix = (uint64_t)width * height, nlo = (uint64_t)lo_width * lo_height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, lo_film_bytes = (size_t)nlo * sizeof(float4), lo_planes_bytes = 3 * lo_film_bytes;
    const size_t mask_bytes = (size_t)npix, ids_bytes = (size_t)npix * sizeof(int4);
    const size_t table_bytes = (size_t)mp->n_prims * sizeof(uint32_t), bodies_bytes = (size_t)mp->n_bodies * 12 * sizeof(float);
    // trhip_temporal_upsample's four, then the three arrays this pass reads beside them (an array whose count is 0 is never read and overlaps nothing)
    const ByteRange ins[7] = {{lo_xyzw, lo_film_bytes}, {lo_planes, lo_planes_bytes}, {hi_planes, planes_bytes}, {history, planes_bytes}, {ids, ids_bytes},
                              {table_bytes ? body_of_prim : nullptr, table_bytes}, {bodies_bytes ? bodies : nullptr, bodies_bytes}};
    if (overlaps_any(out_history, planes_bytes, ins, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_history overlaps an input");
    if (overlaps_any(out, film_bytes, ins, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_xyzw overlaps an input");
    if (overlaps_any(out_mask, mask_bytes, ins, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_mask overlaps an input");
    if (overlap(out, film_bytes, out_history, planes_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_xyzw overlaps out_history");
    if (overlap(out_mask, mask_bytes, out_history, planes_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_mask overlaps out_history");
    if (overlap(out_mask, mask_bytes, out, film_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: out_mask overlaps out_xyzw");
    if (mp->n_prims > 0 && !body_of_prim) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: n_prims = %u but body_of_prim is null", mp->n_prims);
    if (mp->n_prims > 0 && !ids) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: ids may be null only with n_prims = 0, not %u", mp->n_prims);
    if (mp->n_bodies > 0 && !bodies) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample_motion: n_bodies = %u but bodies is null", mp->n_bodies);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    const int R = (int)prm->radius;
    const StagedSquare sq = staged_square(prm->lo_from_hi, R);
    // the host variant's copies: 64 B per low pixel; per full-size pixel planes 48, history 48, new history 48, film 16, ids 16, mask 1; 48 per body, 4 per primitive.  The
    // 16-byte records first, then the table, the mask's bytes last, so that each keeps its alignment in the staging buffer whatever n_prims and the film's size are
    ImageStaging images(ctx, ctx->up_in, is_device);
    const ImageStaging::Image& lo_film = images.input(lo_xyzw, lo_film_bytes);
    const ImageStaging::Image& lo_guides = images.input(lo_planes, lo_planes_bytes);
    const ImageStaging::Image& hi_guides = images.input(hi_planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
    const ImageStaging::Image& result = images.output(out, film_bytes);
    const ImageStaging::Image& id_plane = images.input(ids, ids_bytes);
    const ImageStaging::Image& matrices = images.input(bodies, bodies_bytes);
    const ImageStaging::Image& table = images.input(body_of_prim, table_bytes);
    const ImageStaging::Image& mask = images.output(out_mask, mask_bytes);
    {
        const size_t held = ctx->up_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (bx > 65535u || by > 65535u || lo_width > kUpMaxLowDim || lo_height > kUpMaxLowDim || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_temporal_upsample_motion: the images of a %u x %u film from %u x %u (%.1f GB) do not fit in free HBM (%.1f GB free); there are no bands here",
                        width, height, lo_width, lo_height, need * 1e-9, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const float4 *d_lo = lo_film.in<float4>(), *d_lo_planes = lo_guides.in<float4>(), *d_hi_planes = hi_guides.in<float4>(), *d_history = old_history.in<float4>();
    float4 *d_out = result.out<float4>(), *d_out_history = new_history.out<float4>();
    uint8_t* d_mask = mask.out<uint8_t>();  // NULL when the caller wants none
    // an empty array is never read: the kernel sees it as absent (a staged image of zero bytes has an address all the same)
    const uint32_t* d_table = mp->n_prims ? table.in<uint32_t>() : nullptr;
    const float* d_bodies = mp->n_bodies ? matrices.in<float>() : nullptr;
    const int4* d_ids = mp->n_prims ? id_plane.in<int4>() : nullptr;  // without a table every pixel is static before anything is read
    TemporalUpsampleConst k;
    k.up = upscale_const<UpscaleConst>(prm->lo_from_hi, R, prm->guide_sigma_normal, prm->guide_sigma_plane, prm->min_coverage);  // demodulation and coverage are not offered here
    k.tp = temporal_const<TemporalConst>(*prm);
    k.kappa0 = prm->confidence_floor, k.rho = prm->confidence_sharpness;
    hipStream_t st = ctx->stream;
    const dim3 grid(bx, by), block(kDnTile * kDnTile);
    const int lw = (int)lo_width, lh = (int)lo_height;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    if (R == 1)
        hipLaunchKernelGGL((k_temporal_upsample_motion<1>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, d_history, d_ids, d_table, d_bodies, (int)width,
                           (int)height, k, sq.tw, sq.stride, mp->n_prims, mp->n_bodies, d_out, d_out_history, d_mask);
    else
        hipLaunchKernelGGL((k_temporal_upsample_motion<2>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, d_history, d_ids, d_table, d_bodies, (int)width,
                           (int)height, k, sq.tw, sq.stride, mp->n_prims, mp->n_bodies, d_out, d_out_history, d_mask);
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

}  // namespace

extern "C" {

int trhip_temporal_upsample_motion_default_params(trhip_temporal_upsample_motion_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);  // n_prims = n_bodies = 0: every pixel static
    return trhip_temporal_upsample_default_params(&out->base);
}
int trhip_temporal_upsample_motion(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes, const float* history,
                                   const trhip_aov_id* ids, const uint32_t* body_of_prim, const float* bodies, uint32_t width, uint32_t height,
                                   const trhip_temporal_upsample_motion_params* prm, float* out_xyzw, float* out_history, uint8_t* out_mask, trhip_stats* st) {
    return impl(ctx, lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, history, ids, body_of_prim, bodies, width, height, prm, out_xyzw, out_history, out_mask, false, st);
}
int trhip_temporal_upsample_motion_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes,
                                          const void* d_history, const void* d_ids, const void* d_body_of_prim, const void* d_bodies, uint32_t width, uint32_t height,
                                          const trhip_temporal_upsample_motion_params* prm, void* d_out_xyzw, void* d_out_history, void* d_out_mask, trhip_stats* st) {
    return impl(ctx, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, d_history, d_ids, d_body_of_prim, d_bodies, width, height, prm, d_out_xyzw, d_out_history, d_out_mask, true,
                st);
}

}  // extern "C"
