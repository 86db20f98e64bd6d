// tu_temporal_split.hip — trhip_temporal_split and trhip_film_add: the two passes of th_temporal_split.h.  trhip_temporal_split is trhip_temporal_motion's pass with the frame's
// direct film taken out of the film first; trhip_film_add puts a film's xyz back onto another.  No scene, no traversal: image-space passes on the scaffold of th_image_pass.h.
#include "th_host.h"
#include "th_temporal_split.h"
#include "th_image_pass.h"

#include <cmath>

namespace {

constexpr size_t kSpHostBytesPerPixel = 192;  // the host entry point's copies: film 16, direct 16, planes 48, history 48, new history 48, ids 16 (and 4 per primitive, 48 per body)
constexpr uint32_t kFilmAddMaxBlocks = 2048;  // 256 CUs x 8 blocks of four waves: the grid-stride loop takes the rest

// trhip_temporal_motion's checks of its block, in its order, under this entry's name
int check_params(trhip_ctx* ctx, const trhip_temporal_motion_params* p) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(p->prev_world_to_pixel[i])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: prev_world_to_pixel[%d] is not finite", i);
    if (!(std::isfinite(p->max_history) && p->max_history >= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: max_history must be finite and >= 1");
    if (!positive_finite(p->sigma_normal)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: sigma_normal must be finite and > 0");
    if (!positive_finite(p->sigma_plane)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: sigma_plane must be finite and > 0");
    if (!(p->min_coverage >= 0.0f && p->min_coverage <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: min_coverage must lie in [0, 1]");
    if (p->flags != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: unknown flag bits 0x%x", p->flags);
    if (p->reserved != 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: reserved must be 0");
    return 0;
}

int split_impl(trhip_ctx* ctx, const void* xyzw, const void* direct, const void* planes, const void* history, const void* ids, const void* body_of_prim, const void* bodies, uint32_t width,
               uint32_t height, const trhip_temporal_motion_params* prm, void* out, void* out_history, bool is_device, trhip_stats* stats) {
    // the parameter block first, before any handle is looked at: none of it needs a device
    if (!prm) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (int rc = check_params(ctx, prm)) return rc;
    if (!ctx || !xyzw || !planes || !out || !out_history || (!ids && prm->n_prims > 0)) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: empty film (%u x %u)", width, height);
    if (prm->n_prims > 0 && !body_of_prim) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: n_prims = %u but body_of_prim is null", prm->n_prims);
    if (prm->n_bodies > 0 && !bodies) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: n_bodies = %u but bodies is null", prm->n_bodies);
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4), planes_bytes = 3 * film_bytes, ids_bytes = (size_t)npix * sizeof(int4);
    const size_t table_bytes = (size_t)prm->n_prims * sizeof(uint32_t), bodies_bytes = (size_t)prm->n_bodies * 12 * sizeof(float);
    // trhip_temporal_motion's seven, then the direct film
    const ByteRange frame[8] = {{xyzw, film_bytes}, {planes, planes_bytes}, {history, planes_bytes}, {out, film_bytes}, {ids, ids_bytes}, {table_bytes ? body_of_prim : nullptr, table_bytes},
                                {bodies_bytes ? bodies : nullptr, bodies_bytes}, {direct, film_bytes}};
    if (overlaps_any(out_history, planes_bytes, frame, 7)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: out_history overlaps an input or out_xyzw");
    if (overlaps_any(out, film_bytes, frame + 4, 3)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: out_xyzw overlaps ids, body_of_prim or bodies");
    if (overlaps_any(out_history, planes_bytes, frame + 7, 1)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: out_history overlaps direct");
    if (overlaps_any(out, film_bytes, frame + 7, 1)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_temporal_split: out_xyzw overlaps direct");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t bx = (width + kDnTile - 1) / kDnTile, by = (height + kDnTile - 1) / kDnTile;
    // the images in the order of the host layout: the 16-byte records first, so that each keeps its alignment in the staging buffer whatever n_prims is
    ImageStaging images(ctx, ctx->tp_in, is_device);
    const ImageStaging::Image& film = images.inout(xyzw, out, film_bytes);
    const ImageStaging::Image& direct_film = images.input(direct, film_bytes);
    const ImageStaging::Image& guides = images.input(planes, planes_bytes);
    const ImageStaging::Image& old_history = images.input(history, planes_bytes);
    const ImageStaging::Image& new_history = images.output(out_history, planes_bytes);
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
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_temporal_split: the images of a %u x %u film (%.1f GB, %u B per pixel) do not fit in free HBM (%.1f GB free); there are no bands here",
                        width, height, need * 1e-9, (unsigned)kSpHostBytesPerPixel, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const TemporalConst k = temporal_const<TemporalConst>(*prm);
    // an empty array is never read: the kernel sees it as absent (a staged image of zero bytes has an address all the same)
    const uint32_t* d_table = prm->n_prims ? table.in<uint32_t>() : nullptr;
    const float* d_bodies = prm->n_bodies ? matrices.in<float>() : nullptr;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    hipLaunchKernelGGL(k_temporal_split, dim3(bx, by), dim3(kDnTile * kDnTile), 0, w.st, film.in<float4>(), direct_film.in<float4>(), guides.in<float4>(), old_history.in<float4>(),
                       id_plane.in<int4>(), d_table, d_bodies, (int)width, (int)height, k, prm->n_prims, prm->n_bodies, film.out<float4>(), new_history.out<float4>());
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

int film_add_impl(trhip_ctx* ctx, const void* a, const void* b, uint32_t width, uint32_t height, void* out, bool is_device, trhip_stats* stats) {
    if (!ctx || !a || !b || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (width == 0 || height == 0) return fail(ctx, TRHIP_ERR_INVALID, "trhip_film_add: empty film (%u x %u)", width, height);
    const uint64_t npix = (uint64_t)width * height;
    const size_t film_bytes = (size_t)npix * sizeof(float4);
    if (overlap(out, film_bytes, b, film_bytes)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_film_add: out overlaps b");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ImageStaging images(ctx, ctx->tp_in, is_device);
    const ImageStaging::Image& film = images.inout(a, out, film_bytes);
    const ImageStaging::Image& added = images.input(b, film_bytes);
    {
        const size_t held = ctx->tp_in.bytes;
        const double need = (double)images.bytes();
        bool fits;
        double free_gb;
        if (int rc = fits_in_hbm(ctx, need, held, &fits, &free_gb)) return rc;
        if (!fits)
            return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_film_add: the images of a %u x %u film (%.1f GB, 32 B per pixel) do not fit in free HBM (%.1f GB free); there are no bands here", width,
                        height, need * 1e-9, free_gb);
    }
    if (int rc = images.upload()) return rc;
    const uint64_t blocks = (npix + kFilmAddBlock - 1) / kFilmAddBlock;

    PassWindow w(ctx, stats);
    HIP_TRY(ctx, w.open());
    w.begin(5);
    hipLaunchKernelGGL(k_film_add, dim3((uint32_t)(blocks < kFilmAddMaxBlocks ? blocks : kFilmAddMaxBlocks)), dim3(kFilmAddBlock), 0, w.st, film.in<float4>(), added.in<float4>(), (size_t)npix,
                       film.out<float4>());
    w.end(5);
    return close_pass(ctx, w, images, stats, 1, 1);
}

}  // namespace

extern "C" {

int trhip_temporal_split(trhip_ctx* ctx, const float* xyzw, const float* direct, const float* planes, const float* history, const trhip_aov_id* ids, const uint32_t* body_of_prim,
                         const float* bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* prm, float* out_xyzw, float* out_history, trhip_stats* st) {
    return split_impl(ctx, xyzw, direct, planes, history, ids, body_of_prim, bodies, width, height, prm, out_xyzw, out_history, false, st);
}
int trhip_temporal_split_device(trhip_ctx* ctx, const void* d_xyzw, const void* d_direct, const void* d_planes, const void* d_history, const void* d_ids, const void* d_body_of_prim,
                                const void* d_bodies, uint32_t width, uint32_t height, const trhip_temporal_motion_params* prm, void* d_out_xyzw, void* d_out_history, trhip_stats* st) {
    return split_impl(ctx, d_xyzw, d_direct, d_planes, d_history, d_ids, d_body_of_prim, d_bodies, width, height, prm, d_out_xyzw, d_out_history, true, st);
}
int trhip_film_add(trhip_ctx* ctx, const float* a, const float* b, uint32_t width, uint32_t height, float* out, trhip_stats* st) {
    return film_add_impl(ctx, a, b, width, height, out, false, st);
}
int trhip_film_add_device(trhip_ctx* ctx, const void* d_a, const void* d_b, uint32_t width, uint32_t height, void* d_out, trhip_stats* st) {
    return film_add_impl(ctx, d_a, d_b, width, height, d_out, true, st);
}

}  // extern "C"
