// tu_denoise.hip — trhip_denoise: the edge-avoiding à-trous filter of th_denoise.h on a film and its feature planes.  No scene, no traversal: an image-space pass.
#include "th_host.h"
#include "th_denoise.h"
#include "th_denoise_var.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_denoise_params) == 32, "trhip_denoise_params layout");
static_assert(sizeof(trhip_denoise_var_params) == 48, "trhip_denoise_var_params layout");

constexpr uint32_t kDnMaxIterations = 6;
constexpr size_t kDvBytesPerPixel = 88;  // trhip_denoise_var: the same and V x 2
constexpr size_t kDnBytesPerPixel = 80;  // {n, flag} {p, 0} {c, Y} x 2 {a, 0}

int check_params(trhip_ctx* ctx, const trhip_denoise_params* p) {
    if (p->iterations > kDnMaxIterations) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: iterations = %u, at most %u", p->iterations, kDnMaxIterations);
    if (p->flags & ~(uint32_t)TRHIP_DENOISE_DEMODULATE) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: unknown flag bits 0x%x", p->flags & ~(uint32_t)TRHIP_DENOISE_DEMODULATE);
    if (!positive_finite(p->sigma_colour)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: sigma_colour must be finite and > 0");
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: sigma_plane must be finite and > 0");
    if (!positive_finite(p->albedo_floor)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: albedo_floor must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: min_coverage must lie in [0, 1]");
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: reserved must be 0");
    return 0;
}

int denoise_impl(trhip_ctx* ctx, const void* xyzw, const void* planes, uint32_t width, uint32_t height, const trhip_denoise_params* prm, void* out, bool is_device, trhip_stats* stats) {
    if (!ctx || !xyzw || !planes || !prm || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: empty film (%u x %u)", width, height);
    if (int rc = check_params(ctx, prm)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes;
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    ImageStaging images(ctx, ctx->dn_in, is_device);
    const ImageStaging::Image& film = images.inout(xyzw, out, film_bytes);  // the film's copy is denoised in place
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    {
        const size_t held = ctx->dn_work.bytes + ctx->dn_in.bytes;  // reused below
        const double need = (double)npix * kDnBytesPerPixel + (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (by > 65535u || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_denoise: the working set of a %u x %u film (%.1f GB, 80 B per pixel) does not fit in free HBM (%.1f GB free); there are no bands here", width,
                        height, need * 1e-9, free_gb);
    }
    if (int rc = ensure(ctx, ctx->dn_work, (size_t)npix * kDnBytesPerPixel)) return rc;
    if (int rc = images.upload()) return rc;
    const float4 *d_beauty = film.in<float4>(), *d_planes = guides.in<float4>();
    float4* d_out = film.out<float4>();
    float4* gn = (float4*)ctx->dn_work.p;
    float4 *gp = gn + npix, *col[2] = {gn + 2 * npix, gn + 3 * npix}, *alb = gn + 4 * npix;
    hipStream_t st = ctx->stream;
    const uint32_t demodulate = prm->flags & TRHIP_DENOISE_DEMODULATE;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    if (prm->iterations == 0) {
        if (d_out != d_beauty) HIP_TRY(ctx, hipMemcpyAsync(d_out, d_beauty, film_bytes, hipMemcpyDeviceToDevice, st));
    } else {
        const int lin_grid = grid_for(ctx, npix, 8);
        w.begin(5);
        hipLaunchKernelGGL(k_denoise_prepare, dim3(lin_grid), dim3(kBlock), 0, st, d_beauty, d_planes, npix, demodulate, prm->albedo_floor, prm->min_coverage, gn, gp, col[0], alb);
        w.end(5);
        DenoiseWeights sg{prm->sigma_colour, prm->sigma_normal, prm->sigma_plane};
        for (uint32_t i = 0; i < prm->iterations; ++i) {
            const float4* cin = col[i & 1];
            float4* cout = col[(i & 1) ^ 1];
            const dim3 grid(bx, by), block(kDnTile * kDnTile);
            const bool lds = i < 2 && ((ctx->opt.denoise_lds >> i) & 1);  // steps 1 and 2: measured faster staged, step 4 slower (profiles/r9/denoise.txt)
            w.begin(6);
            if (lds && i == 0)
                hipLaunchKernelGGL((k_denoise_atrous_lds<1>), grid, block, 0, st, gn, gp, cin, cout, (int)width, (int)height, sg);
            else if (lds)
                hipLaunchKernelGGL((k_denoise_atrous_lds<2>), grid, block, 0, st, gn, gp, cin, cout, (int)width, (int)height, sg);
            else
                hipLaunchKernelGGL(k_denoise_atrous, grid, block, 0, st, gn, gp, cin, cout, (int)width, (int)height, 1 << i, sg);
            w.end(6);
            sg.sigma_colour *= 0.5f;
        }
        w.begin(7);
        hipLaunchKernelGGL(k_denoise_finish, dim3(lin_grid), dim3(kBlock), 0, st, d_beauty, gn, col[prm->iterations & 1], alb, npix, demodulate, d_out);
        w.end(7);
    }
    return close_pass(ctx, w, images, stats, 3, kCountedLaunches);  // prepare, the iterations, finish
}

int denoise_var_impl(trhip_ctx* ctx, const void* xyzw, const void* planes, const void* variance, uint32_t width, uint32_t height, const trhip_denoise_var_params* vp, void* out,
                     void* out_variance, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!vp) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    const trhip_denoise_params* prm = &vp->base;
    if (int rc = check_params(ctx, prm)) return rc;
    if (!positive_finite(vp->var_eps)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise_var: var_eps must be finite and > 0");
    if (vp->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise_var: unknown flag bits 0x%x", vp->flags);
    if (vp->reserved[0] != 0 || vp->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise_var: reserved must be 0");
    if (!ctx || !xyzw || !planes || !variance || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_denoise: empty film (%u x %u)", width, height);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, var_bytes = (size_t)npix * sizeof(float);
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    ImageStaging images(ctx, ctx->dn_in, is_device);
    const ImageStaging::Image& film = images.inout(xyzw, out, film_bytes);  // the copies of the film and of the variance plane are filtered in place
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    const ImageStaging::Image& var_plane = images.inout(variance, out_variance, var_bytes);
    {
        const size_t held = ctx->dn_work.bytes + ctx->dn_in.bytes;  // reused below
        const double need = (double)npix * kDvBytesPerPixel + (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (by > 65535u || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_denoise_var: the working set of a %u x %u film (%.1f GB, 88 B per pixel) does not fit in free HBM (%.1f GB free); there are no bands here",
                        width, height, need * 1e-9, free_gb);
    }
    if (int rc = ensure(ctx, ctx->dn_work, (size_t)npix * kDvBytesPerPixel)) return rc;
    if (int rc = images.upload()) return rc;
    const float4 *d_beauty = film.in<float4>(), *d_planes = guides.in<float4>();
    const float* d_variance = var_plane.in<float>();
    float4* d_out = film.out<float4>();
    float* d_out_variance = var_plane.out<float>();  // NULL when the caller wants none
    float4* gn = (float4*)ctx->dn_work.p;
    float4 *gp = gn + npix, *col[2] = {gn + 2 * npix, gn + 3 * npix}, *alb = gn + 4 * npix;
    float* var[2] = {(float*)(gn + 5 * npix), (float*)(gn + 5 * npix) + npix};
    hipStream_t st = ctx->stream;
    const uint32_t demodulate = prm->flags & TRHIP_DENOISE_DEMODULATE;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    const int lin_grid = grid_for(ctx, npix, 8);
    // iterations = 0 copies the film; the variance plane still goes through the seed and the export (clamped, 0 off surfaces), which need the surface flags
    w.begin(5);
    hipLaunchKernelGGL(k_denoise_prepare, dim3(lin_grid), dim3(kBlock), 0, st, d_beauty, d_planes, npix, demodulate, prm->albedo_floor, prm->min_coverage, gn, gp, col[0], alb);
    hipLaunchKernelGGL(k_denoise_var_seed, dim3(lin_grid), dim3(kBlock), 0, st, gn, d_variance, npix, var[0]);
    w.end(5);
    const DenoiseWeights sg{prm->sigma_colour, prm->sigma_normal, prm->sigma_plane};  // sigma_colour multiplies the standard deviation and is not halved
    for (uint32_t i = 0; i < prm->iterations; ++i) {
        const float4* cin = col[i & 1];
        float4* cout = col[(i & 1) ^ 1];
        const float* vin = var[i & 1];
        float* vout = var[(i & 1) ^ 1];
        const dim3 grid(bx, by), block(kDnTile * kDnTile);
        const bool lds = i < 2 && ((ctx->opt.denoise_var_lds >> i) & 1);
        w.begin(6);
        if (lds && i == 0)
            hipLaunchKernelGGL((k_denoise_var_atrous_lds<1>), grid, block, 0, st, gn, gp, cin, vin, cout, vout, (int)width, (int)height, sg, vp->var_eps);
        else if (lds)
            hipLaunchKernelGGL((k_denoise_var_atrous_lds<2>), grid, block, 0, st, gn, gp, cin, vin, cout, vout, (int)width, (int)height, sg, vp->var_eps);
        else
            hipLaunchKernelGGL(k_denoise_var_atrous, grid, block, 0, st, gn, gp, cin, vin, cout, vout, (int)width, (int)height, 1 << i, sg, vp->var_eps);
        w.end(6);
    }
    w.begin(7);
    if (prm->iterations == 0) {
        if (d_out != d_beauty) HIP_TRY(ctx, hipMemcpyAsync(d_out, d_beauty, film_bytes, hipMemcpyDeviceToDevice, st));
    } else
        hipLaunchKernelGGL(k_denoise_finish, dim3(lin_grid), dim3(kBlock), 0, st, d_beauty, gn, col[prm->iterations & 1], alb, npix, demodulate, d_out);
    if (d_out_variance) hipLaunchKernelGGL(k_denoise_var_export, dim3(lin_grid), dim3(kBlock), 0, st, var[prm->iterations & 1], npix, d_out_variance);
    w.end(7);
    return close_pass(ctx, w, images, stats, 3, kCountedLaunches);  // prepare and seed, the iterations, finish and export
}

}  // namespace

extern "C" {

int trhip_denoise_default_params(trhip_denoise_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    out->iterations = 5;
    out->flags = TRHIP_DENOISE_DEMODULATE;
    out->sigma_colour = 4.0f;  // the three sigmas: the sweep of profiles/r9/denoise.txt
    out->sigma_normal = 0.25f;
    out->sigma_plane = 0.1f;
    out->albedo_floor = 1.0f / 64.0f;
    out->min_coverage = 0.5f;
    return 0;
}
int trhip_denoise(trhip_ctx* ctx, const float* xyzw, const float* planes, uint32_t width, uint32_t height, const trhip_denoise_params* prm, float* out_xyzw, trhip_stats* st) {
    return denoise_impl(ctx, xyzw, planes, width, height, prm, out_xyzw, false, st);
}
int trhip_denoise_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, uint32_t width, uint32_t height, const trhip_denoise_params* prm, void* d_out_xyzw, trhip_stats* st) {
    return denoise_impl(ctx, d_xyzw, d_planes, width, height, prm, d_out_xyzw, true, st);
}

int trhip_denoise_var_default_params(trhip_denoise_var_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    if (int rc = trhip_denoise_default_params(&out->base)) return rc;
    // sigma_colour (times the standard deviation), var_eps and trhip_temporal_moments' spatial_below = 4: of the 64 swept cells the one with the lowest geometric mean of the
    // four arc ratios, 0.1461 at max_history 8 (profiles/r13/variance.txt; the unguided session has 0.1445)
    out->base.sigma_colour = 2.0f;
    out->var_eps = 1.0f / 64.0f;
    return 0;
}
int trhip_denoise_var(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* variance, uint32_t width, uint32_t height, const trhip_denoise_var_params* prm, float* out_xyzw,
                      float* out_variance, trhip_stats* st) {
    return denoise_var_impl(ctx, xyzw, planes, variance, width, height, prm, out_xyzw, out_variance, false, st);
}
int trhip_denoise_var_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_variance, uint32_t width, uint32_t height, const trhip_denoise_var_params* prm,
                             void* d_out_xyzw, void* d_out_variance, trhip_stats* st) {
    return denoise_var_impl(ctx, d_xyzw, d_planes, d_variance, width, height, prm, d_out_xyzw, d_out_variance, true, st);
}

}  // extern "C"
