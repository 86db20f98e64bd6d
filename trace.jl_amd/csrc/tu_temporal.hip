// tu_temporal.hip — trhip_temporal: the reprojection pass of th_temporal.h on a film, its feature planes and the previous frame's history; trhip_temporal_clip: the same pass with
// the history clipped to the new frame's neighbourhood colours (th_temporal_clip.h); and trhip_sensor_world_to_pixel, the host arithmetic that gives the pass its matrix.  No
// scene, no traversal: image-space passes.
#include "th_host.h"
#include "th_temporal_clip.h"
#include "th_temporal_moments.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_temporal_params) == 72, "trhip_temporal_params layout");
static_assert(sizeof(trhip_temporal_clip_params) == 88, "trhip_temporal_clip_params layout");
static_assert(sizeof(trhip_temporal_moments_params) == 88, "trhip_temporal_moments_params layout");

constexpr size_t kTpHostBytesPerPixel = 160;  // the host entry point's copies: film 16, planes 48, history 48, new history 48
constexpr size_t kTmHostBytesPerPixel = 196;  // trhip_temporal_moments': trhip_temporal_clip's and moments 8, new moments 8, variance 4
constexpr size_t kTcHostBytesPerPixel = 176;  // trhip_temporal_clip's: the same and a film of its own for the result (the window reads neighbours' film pixels)

int check_params(trhip_ctx* ctx, const trhip_temporal_params* p) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p->prev_world_to_pixel[i])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: prev_world_to_pixel[%d] is not finite", i);
    if (!(std::isfinite(p->max_history) && p->max_history >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: max_history must be finite and >= 1");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: unknown flag bits 0x%x", p->flags);
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: sigma_plane must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: min_coverage must lie in [0, 1]");
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: reserved must be 0");
    return 0;
}

// trhip_temporal's checks on base, in its order, then the new fields
int check_clip_params(trhip_ctx* ctx, const trhip_temporal_clip_params* p) {
    if (int rc = check_params(ctx, &p->base)) return rc;
    if (!(p->clip_gamma >= 0.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip: clip_gamma must be >= 0 (+Inf: no clipping)");  // false for NaN
    if (p->clip_radius < 1 || p->clip_radius > 3) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip: clip_radius must be 1, 2 or 3, not %u", p->clip_radius);
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip: unknown flag bits 0x%x", p->flags);
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_clip: reserved must be 0");
    return 0;
}

// is_clip false: trhip_temporal with prm; true: trhip_temporal_clip with clip, whose base takes prm's place
int temporal_impl(trhip_ctx* ctx, const void* xyzw, const void* planes, const void* history, uint32_t width, uint32_t height, const trhip_temporal_params* prm,
                  const trhip_temporal_clip_params* clip, bool is_clip, void* out, void* out_history, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (is_clip) {
        if (!clip) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
        if (int rc = check_clip_params(ctx, clip)) return rc;
        prm = &clip->base;
    } else {
        if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
        if (int rc = check_params(ctx, prm)) return rc;
    }
    if (!ctx || !xyzw || !planes || !out || !out_history) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: empty film (%u x %u)", width, height);
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes;
    const ByteRange frame[4] = {{xyzw, film_bytes}, {planes, planes_bytes}, {history, planes_bytes}, {out, film_bytes}};
    if (overlaps_any(out_history, planes_bytes, frame, 4)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: out_history overlaps an input or out_xyzw");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    const uint64_t lin_blocks = (npix + kDnTile * kDnTile - 1) / (kDnTile * kDnTile);
    // trhip_temporal accumulates the film where it is: the host variant's copy in place.  The clipping kernel reads the film pixels of a whole window, so it cannot write the film
    // it reads: the host variant has a film of its own for the result, and a device out_xyzw that is (or overlaps) xyzw is written through a film held by the context (16 B per
    // pixel, one device-to-device copy more)
    ImageStaging images(ctx, ctx->tp_in, is_device);
    const ImageStaging::Image& film = is_clip ? images.input(xyzw, film_bytes) : images.inout(xyzw, out, film_bytes);
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
    const ImageStaging::Image& result = is_clip ? images.output_apart(out, film_bytes, film) : film;
    {
        const size_t held = ctx->tp_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (by > 65535u || lin_blocks > 0x7fffffffull || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_temporal: the images of a %u x %u film (%.1f GB, %u B per pixel) do not fit in free HBM (%.1f GB free); there are no bands here", width,
                        height, need * 1e-9, is_clip ? (unsigned)kTcHostBytesPerPixel : (unsigned)kTpHostBytesPerPixel, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const float4 *d_beauty = film.in<float4>(), *d_planes = guides.in<float4>(), *d_history = old_history.in<float4>();
    float4 *d_out = result.out<float4>(), *d_out_history = new_history.out<float4>();
    const TemporalConst k = temporal_const<TemporalConst>(*prm);

    hipStream_t st = ctx->stream;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    if (is_clip) {  // one mapping, the patch's; the option "temporal_patch" has no effect here
        const dim3 grid(bx, by), block(kDnTile * kDnTile);
        const float gamma = clip->clip_gamma;
        if (clip->clip_radius == 1)
            hipLaunchKernelGGL((k_temporal_clip<1>), grid, block, 0, st, d_beauty, d_planes, d_history, (int)width, (int)height, k, gamma, d_out, d_out_history);
        else if (clip->clip_radius == 2)
            hipLaunchKernelGGL((k_temporal_clip<2>), grid, block, 0, st, d_beauty, d_planes, d_history, (int)width, (int)height, k, gamma, d_out, d_out_history);
        else
            hipLaunchKernelGGL((k_temporal_clip<3>), grid, block, 0, st, d_beauty, d_planes, d_history, (int)width, (int)height, k, gamma, d_out, d_out_history);
    } else if (ctx->opt.temporal_patch)  // measured 0.0347 ms against 0.0391 ms at 1024 x 1024 (profiles/r11/temporal.txt)
        hipLaunchKernelGGL((k_temporal<true>), dim3(bx, by), dim3(kDnTile * kDnTile), 0, st, d_beauty, d_planes, d_history, (int)width, (int)height, k, d_out, d_out_history);
    else
        hipLaunchKernelGGL((k_temporal<false>), dim3((uint32_t)lin_blocks), dim3(kDnTile * kDnTile), 0, st, d_beauty, d_planes, d_history, (int)width, (int)height, k, d_out, d_out_history);
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

// trhip_temporal's checks on base, in its order, then the new fields
int check_moments_params(trhip_ctx* ctx, const trhip_temporal_moments_params* p) {
    if (int rc = check_params(ctx, &p->base)) return rc;
    if (!positive_finite(p->albedo_floor)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: albedo_floor must be finite and > 0");
    if (!(std::isfinite(p->spatial_below) && p->spatial_below >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: spatial_below must be finite and >= 1");
    if (p->flags & ~(uint32_t)TRHIP_DENOISE_DEMODULATE)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: unknown flag bits 0x%x", p->flags & ~(uint32_t)TRHIP_DENOISE_DEMODULATE);
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: reserved must be 0");
    return 0;
}

int moments_impl(trhip_ctx* ctx, const void* xyzw, const void* planes, const void* history, const void* moments, uint32_t width, uint32_t height,
                 const trhip_temporal_moments_params* prm, void* out, void* out_history, void* out_moments, void* out_variance, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_moments_params(ctx, prm)) return rc;
    if (!ctx || !xyzw || !planes || !out || !out_history || !out_moments || !out_variance) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: empty film (%u x %u)", width, height);
    if ((history == nullptr) != (moments == nullptr)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: moments must be NULL exactly when history is");
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, mom_bytes = (size_t)npix * sizeof(float2), var_bytes = (size_t)npix * sizeof(float);
    // trhip_temporal's four, then what each further output may not overlap either: out_moments the first six, out_variance all seven
    const ByteRange others[7] = {{xyzw, film_bytes}, {planes, planes_bytes}, {history, planes_bytes}, {out, film_bytes}, {moments, mom_bytes}, {out_history, planes_bytes},
                                 {out_moments, mom_bytes}};
    if (overlaps_any(out_history, planes_bytes, others, 4)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal: out_history overlaps an input or out_xyzw");
    if (overlaps_any(out_moments, mom_bytes, others, 6)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: %s overlaps an input or another output", "out_moments");
    if (overlaps_any(out_variance, var_bytes, others, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: %s overlaps an input or another output", "out_variance");
    if (overlap(out, film_bytes, moments, mom_bytes) || overlap(out_history, planes_bytes, moments, mom_bytes))
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_moments: an output overlaps moments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    // trhip_temporal_clip's images in its layout (the kernel's staging reads the film pixels of a whole window, so out_xyzw is kept apart from xyzw in the same way), then the moments'
    ImageStaging images(ctx, ctx->tp_in, is_device);
    const ImageStaging::Image& film = images.input(xyzw, film_bytes);
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
    const ImageStaging::Image& result = images.output_apart(out, film_bytes, film);
    const ImageStaging::Image& old_moments = images.input(moments, mom_bytes);
    const ImageStaging::Image& new_moments = images.output(out_moments, mom_bytes);
    const ImageStaging::Image& var = images.output(out_variance, var_bytes);
    {
        const size_t held = ctx->tp_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (by > 65535u || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_temporal_moments: the images of a %u x %u film (%.1f GB, %u B per pixel) do not fit in free HBM (%.1f GB free); there are no bands here",
                        width, height, need * 1e-9, (unsigned)kTmHostBytesPerPixel, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const TemporalConst k = temporal_const<TemporalConst>(prm->base);
    const MomentsConst mk{prm->albedo_floor, prm->spatial_below, prm->flags & TRHIP_DENOISE_DEMODULATE};

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    const dim3 grid(bx, by), block(kDnTile * kDnTile);
    hipLaunchKernelGGL(k_temporal_moments, grid, block, 0, w.st, film.in<float4>(), guides.in<float4>(), old_history.in<float4>(), old_moments.in<float2>(), (int)width, (int)height, k, mk,
                       result.out<float4>(), new_history.out<float4>(), new_moments.out<float2>(), var.out<float>());
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

// Gauss-Jordan with partial pivoting on an n x n Float64 matrix (row-major, n <= 4); false when a pivot is zero or not finite.
bool invert(const double* a, int n, double* inv) {
    double m[4][8];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            m[r][c] = a[r * n + c];
            m[r][n + c] = r == c ? 1.0 : 0.0;
        }
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(m[r][c]) > std::fabs(m[piv][c])) piv = r;
        if (!(std::fabs(m[piv][c]) > 0.0) || !std::isfinite(m[piv][c])) return false;
        for (int j = 0; j < 2 * n; ++j) std::swap(m[c][j], m[piv][j]);
        const double d = m[c][c];
        for (int j = 0; j < 2 * n; ++j) m[c][j] /= d;
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = m[r][c];
            for (int j = 0; j < 2 * n; ++j) m[r][j] -= f * m[c][j];
        }
    }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) inv[r * n + c] = m[r][n + c];
    return true;
}

}  // namespace

extern "C" {

// generate_ray (th_kernels.h) sends film position (rx, ry) along the camera-space direction A (rx, ry, 1), A = rows 0-2, columns 0, 1, 3 of raster_to_camera; hence
// (rx, ry, 1) ~ A^-1 (camera_to_world^-1)[rows 0-2] (p, 1).  Film pixel X (1-based, crop_min <= X) has its centre at film position X + 0.5 and array index X - crop_min.
int trhip_sensor_world_to_pixel(const trhip_sensor* sn, float out12[12]) {
    if (!sn || !out12) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    double A[9], Ai[9], C[16], Ci[16];
    for (int r = 0; r < 3; ++r) {
        A[3 * r] = sn->raster_to_camera[4 * r];
        A[3 * r + 1] = sn->raster_to_camera[4 * r + 1];
        A[3 * r + 2] = sn->raster_to_camera[4 * r + 3];
    }
    for (int i = 0; i < 16; ++i) C[i] = sn->camera_to_world[i];
    if (!invert(A, 3, Ai)) return fail(nullptr, TRHIP_ERR_INVALID, "trhip_sensor_world_to_pixel: raster_to_camera is singular");
    if (!invert(C, 4, Ci)) return fail(nullptr, TRHIP_ERR_INVALID, "trhip_sensor_world_to_pixel: camera_to_world is singular");
    double M[3][4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) M[r][c] = (Ai[3 * r] * Ci[c] + Ai[3 * r + 1] * Ci[4 + c]) + Ai[3 * r + 2] * Ci[8 + c];
    for (int c = 0; c < 4; ++c) {
        M[0][c] -= ((double)sn->crop_min[0] + 0.5) * M[2][c];
        M[1][c] -= ((double)sn->crop_min[1] + 0.5) * M[2][c];
    }
    float m[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            m[4 * r + c] = (float)M[r][c];
            if (!std::isfinite(m[4 * r + c])) return fail(nullptr, TRHIP_ERR_INVALID, "trhip_sensor_world_to_pixel: the matrix is not finite in Float32");
        }
    std::memcpy(out12, m, sizeof m);
    return 0;
}

int trhip_temporal_default_params(trhip_temporal_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    // prev_world_to_pixel stays zero: h.z = 0 for every point, so a caller who forgets to fill it gets a frame without history, not a wrong one
    out->max_history = 8.0f;  // the sweep of profiles/r11/temporal.txt: of 8, 16, 32, 64 the shortest did best on a 40-frame arc
    out->sigma_normal = 0.25f;  // the denoiser's geometric sigmas (profiles/r9/denoise.txt)
    out->sigma_plane = 0.1f;
    out->min_coverage = 0.5f;
    return 0;
}
int trhip_temporal(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, uint32_t width, uint32_t height, const trhip_temporal_params* prm, float* out_xyzw,
                   float* out_history, trhip_stats* st) {
    return temporal_impl(ctx, xyzw, planes, history, width, height, prm, nullptr, false, out_xyzw, out_history, false, st);
}
int trhip_temporal_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, uint32_t width, uint32_t height, const trhip_temporal_params* prm, void* d_out_xyzw,
                          void* d_out_history, trhip_stats* st) {
    return temporal_impl(ctx, d_xyzw, d_planes, d_history, width, height, prm, nullptr, false, d_out_xyzw, d_out_history, true, st);
}

int trhip_temporal_clip_default_params(trhip_temporal_clip_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    if (int rc = trhip_temporal_default_params(&out->base)) return rc;
    // the sweep of profiles/r12/temporal_clip.txt (gamma 0.5, 1, 2, 4 x R 1, 2, 3): of the cells that clip, this one has the lowest geometric mean of the four arc ratios at
    // max_history 8 (0.1454; not clipping at all has 0.1445).  Smaller windows and gammas relight faster (0.09 against 0.28 of the unclipped error) and cost more on an arc
    out->clip_gamma = 4.0f;
    out->clip_radius = 3;
    return 0;
}
int trhip_temporal_clip(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, uint32_t width, uint32_t height, const trhip_temporal_clip_params* prm, float* out_xyzw,
                        float* out_history, trhip_stats* st) {
    return temporal_impl(ctx, xyzw, planes, history, width, height, nullptr, prm, true, out_xyzw, out_history, false, st);
}
int trhip_temporal_clip_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, uint32_t width, uint32_t height, const trhip_temporal_clip_params* prm,
                               void* d_out_xyzw, void* d_out_history, trhip_stats* st) {
    return temporal_impl(ctx, d_xyzw, d_planes, d_history, width, height, nullptr, prm, true, d_out_xyzw, d_out_history, true, st);
}

int trhip_temporal_moments_default_params(trhip_temporal_moments_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    if (int rc = trhip_temporal_default_params(&out->base)) return rc;
    out->albedo_floor = 1.0f / 64.0f;  // trhip_denoise_default_params'
    out->spatial_below = 4.0f;         // SVGF's: fewer than four frames of history estimate spatially; 2 measured the same to three digits (profiles/r13/variance.txt)
    out->flags = TRHIP_DENOISE_DEMODULATE;
    return 0;
}
int trhip_temporal_moments(trhip_ctx* ctx, const float* xyzw, const float* planes, const float* history, const float* moments, uint32_t width, uint32_t height,
                           const trhip_temporal_moments_params* prm, float* out_xyzw, float* out_history, float* out_moments, float* out_variance, trhip_stats* st) {
    return moments_impl(ctx, xyzw, planes, history, moments, width, height, prm, out_xyzw, out_history, out_moments, out_variance, false, st);
}
int trhip_temporal_moments_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_planes, const void* d_history, const void* d_moments, uint32_t width, uint32_t height,
                                  const trhip_temporal_moments_params* prm, void* d_out_xyzw, void* d_out_history, void* d_out_moments, void* d_out_variance, trhip_stats* st) {
    return moments_impl(ctx, d_xyzw, d_planes, d_history, d_moments, width, height, prm, d_out_xyzw, d_out_history, d_out_moments, d_out_variance, true, st);
}

}  // extern "C"
