// tu_upscale.hip — trhip_upscale: the joint bilateral upsampling of th_upscale.h from a low-resolution film and its planes onto the planes of the full-size sensor.  No scene, no
// traversal: an image-space pass.
#include "th_host.h"
#include "th_upscale.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_upscale_params) == 48, "trhip_upscale_params layout");

int check_params(trhip_ctx* ctx, const trhip_upscale_params* p) {
    if (int rc = check_lo_from_hi(ctx, "trhip_upscale", p->lo_from_hi)) return rc;
    if (p->radius != 1 && p->radius != 2) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: radius must be 1 or 2, not %u", p->radius);
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: sigma_plane must be finite and > 0");
    if (!positive_finite(p->albedo_floor)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: albedo_floor must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: min_coverage must lie in [0, 1]");
    const uint32_t known = TRHIP_UPSCALE_DEMODULATE | TRHIP_UPSCALE_COVERAGE;
    if (p->flags & ~known) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: unknown flag bits 0x%x", p->flags & ~known);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: reserved must be 0");
    return 0;
}

int upscale_impl(trhip_ctx* ctx, const void* lo_xyzw, const void* lo_planes, uint32_t lo_width, uint32_t lo_height, const void* hi_planes, uint32_t width, uint32_t height,
                 const trhip_upscale_params* prm, void* out, void* out_mask, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, prm)) return rc;
    if (!ctx || !lo_xyzw || !lo_planes || !hi_planes || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0 || lo_width == 0 || lo_height == 0)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: empty image (%u x %u from %u x %u)", width, height, lo_width, lo_height);
    const uint64_t npix = (uint64_t)width * height, nlo = (uint64_t)lo_width * lo_height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, lo_film_bytes = (size_t)nlo * sizeof(float4), lo_planes_bytes = 3 * lo_film_bytes;
    const size_t mask_bytes = (size_t)npix;
    const ByteRange ins[3] = {{lo_xyzw, lo_film_bytes}, {lo_planes, lo_planes_bytes}, {hi_planes, planes_bytes}};
    if (overlaps_any(out, film_bytes, ins, 3)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: out_xyzw overlaps an input");
    if (overlaps_any(out_mask, mask_bytes, ins, 3)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: out_mask overlaps an input");
    if (overlap(out_mask, mask_bytes, out, film_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_upscale: out_mask overlaps out_xyzw");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    const int R = (int)prm->radius;
    const StagedSquare sq = staged_square(prm->lo_from_hi, R);
    // the host variant's copies: 64 B per low pixel, 65 per full-size pixel
    ImageStaging images(ctx, ctx->up_in, is_device);
    const ImageStaging::Image& lo_film = images.input(lo_xyzw, lo_film_bytes);
    const ImageStaging::Image& lo_guides = images.input(lo_planes, lo_planes_bytes);
    const ImageStaging::Image& hi_guides = images.input(hi_planes, planes_bytes);
    const ImageStaging::Image& result = images.output(out, film_bytes);
    const ImageStaging::Image& mask = images.output(out_mask, mask_bytes);
    {
        const size_t held = ctx->up_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (bx > 65535u || by > 65535u || lo_width > kUpMaxLowDim || lo_height > kUpMaxLowDim || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_upscale: the images of a %u x %u film from %u x %u (%.1f GB) do not fit in free HBM (%.1f GB free); there are no bands here", width,
                        height, lo_width, lo_height, need * 1e-9, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const float4 *d_lo = lo_film.in<float4>(), *d_lo_planes = lo_guides.in<float4>(), *d_hi_planes = hi_guides.in<float4>();
    float4* d_out = result.out<float4>();
    uint8_t* d_mask = mask.out<uint8_t>();  // NULL when the caller wants none
    UpscaleConst k = upscale_const<UpscaleConst>(prm->lo_from_hi, R, prm->sigma_normal, prm->sigma_plane, prm->min_coverage);
    k.demodulate = prm->flags & TRHIP_UPSCALE_DEMODULATE;
    k.coverage = prm->flags & TRHIP_UPSCALE_COVERAGE;
    k.albedo_floor = prm->albedo_floor;
    hipStream_t st = ctx->stream;
    const dim3 grid(bx, by), block(kDnTile * kDnTile);
    const int lw = (int)lo_width, lh = (int)lo_height;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    if (R == 1)
        hipLaunchKernelGGL((k_upscale<1>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, (int)width, (int)height, k, sq.tw, sq.stride, d_out, d_mask);
    else
        hipLaunchKernelGGL((k_upscale<2>), grid, block, sq.lds_bytes, st, d_lo, d_lo_planes, lw, lh, d_hi_planes, (int)width, (int)height, k, sq.tw, sq.stride, d_out, d_mask);
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

}  // namespace

extern "C" {

int trhip_upscale_default_params(trhip_upscale_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    // lo_from_hi stays zero: a scale of 0 is refused, so a caller who forgets the map gets an error, not a smeared frame
    // radius, flags and sigma_plane: of the swept cells (R 1, 2 x both flags on / off x sigma_plane 0.1, 0.2, 0.4 x the denoiser before or after) the one with the lowest geometric
    // mean of the two scenes' error ratios to the native frame, 1.065 (profiles/r14/upscale.txt); with both flags on the best cell has 1.161
    out->radius = 2;
    out->flags = 0;
    out->sigma_normal = 0.25f;  // the denoiser's (profiles/r9/denoise.txt)
    out->sigma_plane = 0.4f;
    out->albedo_floor = 1.0f / 64.0f;
    out->min_coverage = 0.5f;
    return 0;
}
int trhip_upscale(trhip_ctx* ctx, const float* lo_xyzw, const float* lo_planes, uint32_t lo_width, uint32_t lo_height, const float* hi_planes, uint32_t width, uint32_t height,
                  const trhip_upscale_params* prm, float* out_xyzw, uint8_t* out_mask, trhip_stats* st) {
    return upscale_impl(ctx, lo_xyzw, lo_planes, lo_width, lo_height, hi_planes, width, height, prm, out_xyzw, out_mask, false, st);
}
int trhip_upscale_device(trhip_ctx* ctx, const void* d_lo_xyzw, const void* d_lo_planes, uint32_t lo_width, uint32_t lo_height, const void* d_hi_planes, uint32_t width, uint32_t height,
                         const trhip_upscale_params* prm, void* d_out_xyzw, void* d_out_mask, trhip_stats* st) {
    return upscale_impl(ctx, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, width, height, prm, d_out_xyzw, d_out_mask, true, st);
}

}  // extern "C"
