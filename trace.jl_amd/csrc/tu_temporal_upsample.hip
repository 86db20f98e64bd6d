// tu_temporal_upsample.hip — trhip_temporal_upsample: the fused upscale-and-accumulate pass of th_temporal_upsample.h from a jittered low-resolution film and its planes, the
// planes of the full-size sensor and the previous frame's full-size history.  No scene, no traversal: an image-space pass.
#include "th_host.h"
#include "th_temporal_upsample.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_temporal_upsample_params) == 112, "trhip_temporal_upsample_params layout");

// trhip_upscale's checks in its order for the fields that are its own, then trhip_temporal's for the rest, then the two new fields
int check_params(trhip_ctx* ctx, const trhip_temporal_upsample_params* p) {
    if (int rc = check_lo_from_hi(ctx, "trhip_temporal_upsample", p->lo_from_hi)) return rc;
    if (p->radius != 1 && p->radius != 2) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: radius must be 1 or 2, not %u", p->radius);
    if (!positive_finite(p->guide_sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: guide_sigma_normal must be finite and > 0");
    if (!positive_finite(p->guide_sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: guide_sigma_plane must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: min_coverage must lie in [0, 1]");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: unknown flag bits 0x%x (demodulation and coverage are not offered here)", p->flags);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: reserved must be 0");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p->prev_world_to_pixel[i])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: prev_world_to_pixel[%d] is not finite", i);
    if (!(std::isfinite(p->max_history) && p->max_history >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: max_history must be finite and >= 1");
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: sigma_plane must be finite and > 0");
    if (!(p->confidence_floor > 0.0f && p->confidence_floor <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: confidence_floor must lie in (0, 1]");
    if (!(p->confidence_sharpness >= 0.0f && p->confidence_sharpness <= 4.0f))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: confidence_sharpness must lie in [0, 4]");
    return 0;
}

int impl(trhip_ctx* ctx, const void* lo_xyzw, const void* lo_planes, uint32_t lo_width, uint32_t lo_height, const void* hi_planes, const void* history, uint32_t width, uint32_t height,
         const trhip_temporal_upsample_params* prm, void* out, void* out_history, void* out_mask, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, prm)) return rc;
    if (!ctx || !lo_xyzw || !lo_planes || !hi_planes || !out || !out_history) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0 || lo_width == 0 || lo_height == 0)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: empty image (%u x %u from %u x %u)", width, height, lo_width, lo_height);
    const uint64_t npix = (uint64_t)width * height, nlo = (uint64_t)lo_width * lo_height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, lo_film_bytes = (size_t)nlo * sizeof(float4), lo_planes_bytes = 3 * lo_film_bytes;
    const size_t mask_bytes = (size_t)npix;
    const ByteRange ins[4] = {{lo_xyzw, lo_film_bytes}, {lo_planes, lo_planes_bytes}, {hi_planes, planes_bytes}, {history, planes_bytes}};
    if (overlaps_any(out_history, planes_bytes, ins, 4)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_history overlaps an input");
    if (overlaps_any(out, film_bytes, ins, 4)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_xyzw overlaps an input");
    if (overlaps_any(out_mask, mask_bytes, ins, 4)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_mask overlaps an input");
    if (overlap(out, film_bytes, out_history, planes_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_xyzw overlaps out_history");
    if (overlap(out_mask, mask_bytes, out_history, planes_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_mask overlaps out_history");
    if (overlap(out_mask, mask_bytes, out, film_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_upsample: out_mask overlaps out_xyzw");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    const int R = (int)prm->radius;
    const StagedSquare sq = staged_square(prm->lo_from_hi, R);
    // the host variant's copies: 64 B per low pixel; per full-size pixel planes 48, history 48, new history 48, film 16, mask 1
    ImageStaging images(ctx, ctx->up_in, is_device);
    const ImageStaging::Image& lo_film = images.input(lo_xyzw, lo_film_bytes);
    const ImageStaging::Image& lo_guides = images.input(lo_planes, lo_planes_bytes);
    const ImageStaging::Image& hi_guides = images.input(hi_planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
    const ImageStaging::Image& result = images.output(out, film_bytes);
    const ImageStaging::Image& mask = images.output(out_mask, mask_bytes);
    {
        const size_t held = ctx->up_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (bx > 65535u || by > 65535u || lo_width > kUpMaxLowDim || lo_height > kUpMaxLowDim || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_temporal_upsample: the images of a %u x %u film from %u x %u (%.1f GB) do not fit in free HBM (%.1f GB free); there are no bands here",
                        width, height, lo_width, lo_height, need * 1e-9, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const float4 *d_lo = lo_film.in<float4>(), *d_lo_planes = lo_guides.in<float4>(), *d_hi_planes = hi_guides.in<float4>(), *d_history = old_history.in<float4>();
    float4 *d_out = result.out<float4>(), *d_out_history = new_history.out<float4>();
    uint8_t* d_mask = mask.out<uint8_t>();  // NULL when the caller wants none
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
        hipLaunchKernelGGL((k_temporal_upsample<1>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, d_history, (int)width, (int)height, k, sq.tw, sq.stride, d_out,
                           d_out_history, d_mask);
    else
        hipLaunchKernelGGL((k_temporal_upsample<2>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, d_history, (int)width, (int)height, k, sq.tw, sq.stride, d_out,
                           d_out_history, d_mask);
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

}  // namespace

extern "C" {

int trhip_temporal_upsample_default_params(trhip_temporal_upsample_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    // lo_from_hi stays zero (a scale of 0 is refused: the map has to be given); prev_world_to_pixel stays zero (h.z = 0 for every point: frames without history, not wrong ones)
    out->max_history = 8.0f;  // trhip_temporal's, and the sweep's (below)
    out->sigma_normal = 0.25f;  // the history taps: trhip_temporal's
    out->sigma_plane = 0.1f;
    out->min_coverage = 0.5f;
    out->guide_sigma_normal = 0.25f;  // the low taps: trhip_upscale's
    out->guide_sigma_plane = 0.4f;
    // radius, max_history, confidence_sharpness and confidence_floor: of the swept cells (R 1, 2 x max_history 8, 16, 32 x rho 0, 1, 2 x kappa_0 1/16, 1/4, 1) the one with the
    // lowest geometric mean of the four error ratios to the upscaled session, 0.617 (profiles/r16/temporal_upsample.txt); 16 and 32 give the same figures to four digits (the
    // accumulated weight does not reach 8 within the 16 frames of the sequences), so the shortest history; the best cell with R = 2 has 0.969
    out->confidence_floor = 0.0625f;
    out->confidence_sharpness = 2.0f;
    out->radius = 1;
    return 0;
}
int trhip_temporal_upsample(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes, const float* history,
                            uint32_t width, uint32_t height, const trhip_temporal_upsample_params* prm, float* out_xyzw, float* out_history, uint8_t* out_mask, trhip_stats* st) {
    return impl(ctx, lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, history, width, height, prm, out_xyzw, out_history, out_mask, false, st);
}
int trhip_temporal_upsample_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes, const void* d_history,
                                   uint32_t width, uint32_t height, const trhip_temporal_upsample_params* prm, void* d_out_xyzw, void* d_out_history, void* d_out_mask, trhip_stats* st) {
    return impl(ctx, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, d_history, width, height, prm, d_out_xyzw, d_out_history, d_out_mask, true, st);
}

}  // extern "C"
