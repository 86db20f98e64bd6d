// tu_display.hip — trhip_display: the display pass of th_display.h on a film state: metering histogram, exposure, tone curve, 8-bit RGBA.  No scene, no traversal: an
// image-space pass, the last of a preview.
#include "th_host.h"
#include "th_display.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

static_assert(sizeof(trhip_display_params) == 48, "trhip_display_params layout");
static_assert(sizeof(trhip_display_state) == 16 && sizeof(DisplayState) == 16, "trhip_display_state layout");

const float h_srgb_thresholds[256] = {TH_SRGB_THRESHOLDS};
constexpr size_t kHistBytes = kDisplayBins * sizeof(uint32_t);  // ctx->dp_work: the histogram, then a state slot for a caller who keeps none
constexpr size_t kWorkBytes = kHistBytes + sizeof(DisplayState);

int check_params(trhip_ctx* ctx, const trhip_display_params* p, float scale) {
    if (p->curve > TRHIP_DISPLAY_CURVE_ACES) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: curve must be 0 (clamp), 1 (Reinhard) or 2 (ACES), not %u", p->curve);
    if (p->transfer > TRHIP_DISPLAY_TRANSFER_SRGB) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: transfer must be 0 (linear) or 1 (sRGB), not %u", p->transfer);
    const uint32_t known = TRHIP_DISPLAY_AUTO_EXPOSURE | TRHIP_DISPLAY_FLIP_ROWS;
    if (p->flags & ~known) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: unknown flag bits 0x%x", p->flags & ~known);
    if (!positive_finite(p->exposure)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: exposure must be finite and > 0");
    if (!positive_finite(p->key)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: key must be finite and > 0");
    if (!positive_finite(p->min_exposure)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: min_exposure must be finite and > 0");
    if (!positive_finite(p->max_exposure)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: max_exposure must be finite and > 0");
    if (p->min_exposure > p->max_exposure) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: min_exposure exceeds max_exposure");
    if (p->percentile_permille < 1 || p->percentile_permille > 1000)
        return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: percentile_permille must lie in 1..1000, not %u", p->percentile_permille);
    if (!(p->adapt_rate > 0.0f && p->adapt_rate <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: adapt_rate must lie in (0, 1]");
    if (!(p->white >= 0.0009765625f && p->white <= 1048576.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: white must lie in [2^-10, 2^20]");
    if (!std::isfinite(scale)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: scale is not finite");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: reserved must be 0");
    return 0;
}

template <int CURVE>
void launch_encode(uint32_t transfer, dim3 grid, dim3 block, hipStream_t st, const float4* in, int w, int h, const DisplayEncodeConst& k, const DisplayState* state, uint32_t* out) {
    if (transfer == TRHIP_DISPLAY_TRANSFER_SRGB)
        hipLaunchKernelGGL((k_display_encode<CURVE, 1>), grid, block, 0, st, in, w, h, k, state, out);
    else
        hipLaunchKernelGGL((k_display_encode<CURVE, 0>), grid, block, 0, st, in, w, h, k, state, out);
}

int display_impl(trhip_ctx* ctx, const void* xyzw, uint32_t width, uint32_t height, float scale, const trhip_display_params* prm, void* state, void* out_rgba, void* out_hist,
                 bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, prm, scale)) return rc;
    if (!ctx || !xyzw || !out_rgba) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: empty image (%u x %u)", width, height);
    const uint64_t npix = (uint64_t)width * height;
    if (npix >= (uint64_t)1 << 31) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: %u x %u pixels, the pass takes fewer than 2^31", width, height);
    const size_t film_bytes = (size_t)npix * sizeof(float4), rgba_bytes = (size_t)npix * 4;
    if (overlap(out_rgba, rgba_bytes, xyzw, film_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_display: out_rgba overlaps the input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    ImageStaging images(ctx, ctx->dp_in, is_device);
    const ImageStaging::Image& film = images.input(xyzw, film_bytes);
    const ImageStaging::Image& rgba = images.output(out_rgba, rgba_bytes);
    {
        const size_t held = ctx->dp_in.bytes;  // reused below
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (bx > 65535u || by > 65535u || !fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_display: the images of a %u x %u film (%.1f GB) do not fit in free HBM (%.1f GB free); there are no bands here", width, height,
                        need * 1e-9, free_gb);
    }
    const bool automatic = (prm->flags & TRHIP_DISPLAY_AUTO_EXPOSURE) != 0;
    if (int rc = ensure(ctx, ctx->dp_work, kWorkBytes)) return rc;
    uint32_t* d_hist = (uint32_t*)ctx->dp_work.p;
    DisplayState* d_slot = (DisplayState*)((char*)ctx->dp_work.p + kHistBytes);
    if (int rc = images.upload()) return rc;
    const float4* d_in = film.in<float4>();
    uint32_t* d_out = rgba.out<uint32_t>();
    DisplayState* d_state = (DisplayState*)state;  // the device variant's, or null
    uint32_t* d_out_hist = (uint32_t*)out_hist;    // likewise
    hipStream_t st = ctx->stream;
    if (!is_device) {  // the 16-byte state and the histogram are not images: they live in dp_work
        d_state = nullptr;
        d_out_hist = nullptr;  // the host reads the context's histogram itself
        if (automatic && state) HIP_TRY(ctx, hipMemcpy(d_slot, state, sizeof(DisplayState), hipMemcpyHostToDevice));
    }
    const bool own_slot = !d_state;  // the state lives in the context's slot for this call
    const bool slot_filled = !is_device && state;
    if (own_slot) d_state = d_slot;

    DisplayResolveConst rk;
    rk.exposure = prm->exposure, rk.key = prm->key, rk.adapt_rate = prm->adapt_rate, rk.min_exposure = prm->min_exposure, rk.max_exposure = prm->max_exposure;
    rk.permille = prm->percentile_permille;
    DisplayEncodeConst ek;
    ek.scale = scale;
    ek.exposure = prm->exposure;
    ek.ww = prm->white * prm->white;
    ek.flip = (prm->flags & TRHIP_DISPLAY_FLIP_ROWS) ? 1u : 0u;
    const dim3 grid(bx, by), block(kDnTile * kDnTile);
    // the meter's grid: one block of 256 lanes per CU, never more than the frame has.  Its time is that of the global adds that end it, blocks x non-empty bins of them:
    // 0.013 ms at 1024^2 against 0.044 at eight blocks per CU (th_display.h, profiles/r15/display.txt)
    const uint32_t meter_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((npix + 255) / 256, (uint64_t)ctx->num_cu));

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    if (automatic) {
        // histogram, and the slot when it stands for "no state"
        HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, own_slot && !slot_filled ? kWorkBytes : kHistBytes, st));
        w.begin(5);
        hipLaunchKernelGGL(k_display_meter, dim3(meter_blocks), dim3(256), 0, st, d_in, (uint32_t)npix, scale, d_hist);
        w.end(5);
        w.begin(6);
        hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(64), 0, st, d_hist, rk, d_state, d_out_hist);
        w.end(6);
    } else if (d_out_hist) {
        HIP_TRY(ctx, hipMemsetAsync(d_out_hist, 0, kHistBytes, st));
    }
    const DisplayState* e_state = automatic ? d_state : nullptr;
    w.begin(7);
    if (prm->curve == TRHIP_DISPLAY_CURVE_CLAMP)
        launch_encode<0>(prm->transfer, grid, block, st, d_in, (int)width, (int)height, ek, e_state, d_out);
    else if (prm->curve == TRHIP_DISPLAY_CURVE_REINHARD)
        launch_encode<1>(prm->transfer, grid, block, st, d_in, (int)width, (int)height, ek, e_state, d_out);
    else
        launch_encode<2>(prm->transfer, grid, block, st, d_in, (int)width, (int)height, ek, e_state, d_out);
    w.end(7);
    if (int rc = close_pass(ctx, w, images, stats, 3, automatic ? 3 : 1)) return rc;  // meter, resolve, encode
    if (!is_device) {
        if (automatic && state) HIP_TRY(ctx, hipMemcpy(state, d_slot, sizeof(DisplayState), hipMemcpyDeviceToHost));
        if (out_hist) {
            if (automatic)
                HIP_TRY(ctx, hipMemcpy(out_hist, d_hist, kHistBytes, hipMemcpyDeviceToHost));
            else
                std::memset(out_hist, 0, kHistBytes);
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int trhip_display_default_params(trhip_display_params* out) {
    if (!out) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    // conventional values, none of them swept: there is no error metric for a tone curve here
    out->curve = TRHIP_DISPLAY_CURVE_REINHARD;
    out->transfer = TRHIP_DISPLAY_TRANSFER_SRGB;
    out->flags = TRHIP_DISPLAY_AUTO_EXPOSURE | TRHIP_DISPLAY_FLIP_ROWS;
    out->exposure = 1.0f;
    out->key = 0.18f;  // the photographic middle grey
    out->percentile_permille = 500;
    out->adapt_rate = 1.0f;
    out->min_exposure = 0.00390625f;  // 2^-8
    out->max_exposure = 256.0f;
    out->white = 4.0f;
    return 0;
}
int trhip_display_srgb_table(float* out256) {
    if (!out256) return fail(nullptr, TRHIP_ERR_INVALID, "null argument");
    std::memcpy(out256, h_srgb_thresholds, sizeof h_srgb_thresholds);
    return 0;
}
int trhip_display(trhip_ctx* ctx, const float* xyzw, uint32_t width, uint32_t height, float scale, const trhip_display_params* prm, trhip_display_state* host_state_inout,
                  uint8_t* out_rgba, uint32_t* out_histogram256, trhip_stats* st) {
    return display_impl(ctx, xyzw, width, height, scale, prm, host_state_inout, out_rgba, out_histogram256, false, st);
}
int trhip_display_device(trhip_ctx* ctx, const void* d_xyzw, uint32_t width, uint32_t height, float scale, const trhip_display_params* prm, void* d_state, void* d_out_rgba,
                         void* d_histogram256, trhip_stats* st) {
    return display_impl(ctx, d_xyzw, width, height, scale, prm, d_state, d_out_rgba, d_histogram256, true, st);
}

}  // extern "C"
