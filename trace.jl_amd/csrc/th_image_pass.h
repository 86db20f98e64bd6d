// th_image_pass.h — the host scaffold of the image-space passes of a preview: tu_denoise.hip, tu_temporal.hip, tu_upscale.hip, tu_display.hip, tu_temporal_upsample.hip,
// tu_temporal_motion.hip, tu_temporal_clip_motion.hip, tu_temporal_upsample_motion.hip and tu_temporal_split.hip, and nobody else.  Host code only: no kernel lives here and
// no kernel header is included, so the units instantiate what they instantiated before.  What a pass keeps to itself: its
// parameter checks, its refusal sentences, its launches.  What it gets from here: where its images live (ImageStaging), whether two of them overlap, the timed window around
// its launches and the block that closes it (PassWindow, close_pass), and the derivations two passes share.  Everything above "the timed window" is arithmetic on the
// arguments and needs no device.
#pragma once
#include "th_host.h"

#include <cassert>
#include <cmath>

inline bool positive_finite(float v) { return std::isfinite(v) && v > 0.0f; }

// ---- overlaps ------------------------------------------------------------------------------------------------------------------------
// Two byte ranges share a byte.  A NULL image overlaps nothing; adjacent ranges do not overlap.
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
struct ByteRange {
    const void* p;
    size_t n;
};
// "this output may overlap none of these images": the first `count` entries of a pass's table
inline bool overlaps_any(const void* p, size_t n, const ByteRange* images, int count) {
    for (int i = 0; i < count; ++i)
        if (overlap(p, n, images[i].p, images[i].n)) return true;
    return false;
}

// ---- where a pass's images live ----------------------------------------------------------------------------------------------------------
// A pass tells the staging each image once, in the order of its host layout, and reads the device pointers from what it gets back.  With device pointers (`is_device`) they
// pass through.  With host pointers every image gets its place in `buf`, one after the other (NULL ones too: the layout, and the bytes the refusal sentences state, do not
// depend on which optional images a caller leaves out), upload() copies the inputs there and download() brings the outputs back.  bytes() is what upload() will ask of `buf`:
// known before anything is allocated, for the HBM check.  Declaring images touches no device.
class ImageStaging {
  public:
    struct Image {
        const void* h_in = nullptr;  // the caller's pointers: read from, written to (either may be NULL)
        void* h_out = nullptr;
        size_t bytes = 0, offset = 0;
        bool staged = false;  // lives in buf (valid after upload()); otherwise the caller's pointers are the device pointers
        const void* d_in = nullptr;
        void* d_out = nullptr;
        template <class T>
        const T* in() const {
            return (const T*)d_in;
        }
        template <class T>
        T* out() const {
            return (T*)d_out;
        }
    };
    static constexpr int kMaxImages = 10;  // trhip_temporal_upsample_motion's ten

    ImageStaging(trhip_ctx* ctx, DevBuf& buf, bool is_device) : ctx_(ctx), buf_(buf), is_device_(is_device) {}
    ImageStaging(const ImageStaging&) = delete;
    ImageStaging& operator=(const ImageStaging&) = delete;

    Image& input(const void* in, size_t bytes) { return add(in, nullptr, bytes, !is_device_); }  // NULL: the pass sees NULL
    Image& output(void* out, size_t bytes) { return add(nullptr, out, bytes, !is_device_); }    // NULL: the pass sees NULL and nothing comes back
    // one image read and written in place.  The host variant's copy is both; device pointers stay the caller's two, which may be equal
    Image& inout(const void* in, void* out, size_t bytes) { return add(in, out, bytes, !is_device_); }
    // an output whose kernel also reads `from` around the pixel it writes, so it cannot write it in place: a device pointer that overlaps from's is written in buf instead and
    // copied to the caller's by finish().  The host variant's copies never overlap
    Image& output_apart(void* out, size_t bytes, const Image& from) { return add(nullptr, out, bytes, !is_device_ || overlap(out, bytes, from.h_in, from.bytes)); }

    size_t bytes() const { return total_; }
    int upload() {
        if (total_ == 0) return 0;
        if (int rc = ensure(ctx_, buf_, total_)) return rc;
        for (int i = 0; i < n_; ++i) {
            Image& im = img_[i];
            if (!im.staged) continue;
            char* p = (char*)buf_.p + im.offset;
            if (!is_device_ && im.h_in) HIP_TRY(ctx_, hipMemcpy(p, im.h_in, im.bytes, hipMemcpyHostToDevice));
            im.d_in = im.h_in ? p : nullptr;
            im.d_out = im.h_out ? p : nullptr;
        }
        return 0;
    }
    // in the stream, after the launches: the device variant's outputs that were written in buf go to the caller's pointers
    int finish(hipStream_t st) {
        for (int i = 0; i < n_ && is_device_; ++i)
            if (img_[i].staged && img_[i].h_out) HIP_TRY(ctx_, hipMemcpyAsync(img_[i].h_out, img_[i].d_out, img_[i].bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    // after the stream has been synchronised
    int download() {
        for (int i = 0; i < n_ && !is_device_; ++i)
            if (img_[i].h_out) HIP_TRY(ctx_, hipMemcpy(img_[i].h_out, img_[i].d_out, img_[i].bytes, hipMemcpyDeviceToHost));
        return 0;
    }

  private:
    Image& add(const void* in, void* out, size_t bytes, bool staged) {
        assert(n_ < kMaxImages);
        Image& im = img_[n_++];
        im.h_in = in, im.h_out = out, im.bytes = bytes, im.staged = staged;
        if (staged) {
            im.offset = total_;
            total_ += bytes;
        } else {
            im.d_in = in, im.d_out = out;
        }
        return im;
    }
    trhip_ctx* ctx_;
    DevBuf& buf_;
    bool is_device_;
    Image img_[kMaxImages];
    int n_ = 0;
    size_t total_ = 0;
};

// ---- derivations two passes share ----------------------------------------------------------------------------------------------------
// (templates where the result is a kernel header's type: this header includes none of them)
// TemporalConst from a parameter block with trhip_temporal_params' fields (trhip_temporal_upsample_params has them under the same names)
template <class TemporalConstT, class Params>
TemporalConstT temporal_const(const Params& p) {
    TemporalConstT k;
    std::memcpy(k.m, p.prev_world_to_pixel, sizeof k.m);
    k.max_history = p.max_history;
    k.sigma_normal = p.sigma_normal;
    k.sigma_plane = p.sigma_plane;
    k.min_coverage = p.min_coverage;
    return k;
}

constexpr uint32_t kUpMaxLowDim = 1u << 24;  // the upscaling passes: low-image indices are ints; positions stay below 2^21 (th_upscale.h)

// trhip_upscale_params.lo_from_hi = (ax, bx, ay, by), as the upscaling passes accept it; `entry` names the entry point in the sentence
inline int check_lo_from_hi(trhip_ctx* ctx, const char* entry, const float* m) {
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(m[i])) return fail(ctx, TRHIP_ERR_INVALID, "%s: lo_from_hi[%d] is not finite", entry, i);
    for (int i = 0; i < 4; i += 2) {
        if (!(m[i] >= 0.25f && m[i] <= 1.0f)) return fail(ctx, TRHIP_ERR_INVALID, "%s: lo_from_hi[%d] = %g, the scale must lie in [1/4, 1]", entry, i, (double)m[i]);
        if (!(std::fabs(m[i + 1]) < 1048576.0f)) return fail(ctx, TRHIP_ERR_INVALID, "%s: lo_from_hi[%d], the offset, must be below 2^20 in magnitude", entry, i + 1);
    }
    return 0;
}
// the square of low pixels a block of the upscaling kernels stages in LDS (th_upscale.h): ceil(15 a) + 1 + 2 R positions per axis, the larger axis deciding
struct StagedSquare {
    int tw, stride;
    size_t lds_bytes;  // at most 40960
};
inline StagedSquare staged_square(const float* lo_from_hi, int R) {
    const float amax = std::fmax(lo_from_hi[0], lo_from_hi[2]);
    StagedSquare s;
    s.tw = (int)std::ceil(15.0 * (double)amax) + 1 + 2 * R;
    s.stride = s.tw <= 16 ? 16 : 32;
    s.lds_bytes = (size_t)4 * s.tw * s.stride * 16;  // four float4 records per position
    return s;
}
// UpscaleConst with the map, the radius and the guide's widths; demodulate, coverage and albedo_floor stay 0 for the pass that offers them to set
template <class UpscaleConstT>
UpscaleConstT upscale_const(const float* lo_from_hi, int R, float sigma_normal, float sigma_plane, float min_coverage) {
    UpscaleConstT k{};
    k.ax = lo_from_hi[0], k.bx = lo_from_hi[1], k.ay = lo_from_hi[2], k.by = lo_from_hi[3];
    k.inv_r = 1.0f / (float)R;
    k.sigma_normal = sigma_normal, k.sigma_plane = sigma_plane, k.min_coverage = min_coverage;
    return k;
}

// ---- the timed window and its close --------------------------------------------------------------------------------------------------------
// The events around a pass's device work (trhip_stats.ms_total) and the Timer of its launches, classes 5-7, on the context's stream.
struct PassWindow {
    Timer tm;
    FrameEvents ev;
    hipStream_t st;
    PassWindow(trhip_ctx* ctx, const trhip_stats* stats) : tm(ctx, ctx->opt.timing && stats), st(ctx->stream) {
        ctx->last.drop_env_records();  // an image pass between a path-env frame and its relight: the relight is refused (include/tracehip.h, trhip_path_env_relight)
    }
    hipError_t open() { return ev.begin(st); }
    void begin(int cls) { tm.begin(cls, st); }
    void end(int cls) { tm.end(cls, st); }
};
// After the last launch: the staging's copies in the stream, the end event, the launches' error, the synchronise, the copies back to the host, the stats.
// parts 1: one launch in class 5, ms_film its time.  parts 3: classes 5-7 in ms_sub / launches_sub [0-2], ms_film their sum.
// launches_film is `launches_film` (a pass that knows the number says it: the Timer counts nothing when timing is off), or what the Timer counted over the three classes.
constexpr int kCountedLaunches = -1;
inline int close_pass(trhip_ctx* ctx, PassWindow& w, ImageStaging& images, trhip_stats* stats, int parts, int launches_film) {
    if (int rc = images.finish(w.st)) return rc;
    HIP_TRY(ctx, w.ev.end(w.st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(w.st));
    if (int rc = images.download()) return rc;
    if (!stats) return 0;
    std::memset(stats, 0, sizeof *stats);
    stats->ms_total = w.ev.ms();
    if (parts == 1)
        stats->ms_film = w.tm.total(5, &stats->launches_film);
    else
        for (int k = 0; k < 3; ++k) {
            stats->ms_sub[k] = w.tm.total(5 + k, &stats->launches_sub[k]);
            stats->ms_film += stats->ms_sub[k];
        }
    stats->launches_film = launches_film >= 0 ? (uint32_t)launches_film : stats->launches_sub[0] + stats->launches_sub[1] + stats->launches_sub[2];
    return 0;
}
