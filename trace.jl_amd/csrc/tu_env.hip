// tu_env.hip — the environment map (trhip_env_create / _free / _size / _eval; th_env.h, docs/design/25-sky.md): the checks, the gutter, the upload, and the lookup on its own.
#include "th_env.h"

#include <cmath>

static_assert(!std::is_copy_constructible_v<trhip_env>, "trhip_env (th_env.h) owns its texels: trhip_env_free is `delete`");

namespace {

constexpr uint32_t kEnvMaxN = 4096;

// The map with its gutter: storage texel (I, J) is the map's (I - 1, J - 1).  A column outside [0, n) takes the interior texel (clamp(i), n - 1 - j), a row outside
// (n - 1 - i, clamp(j)), a corner one rule after the other: the octahedral edge wrap (crossing an edge of the square mirrors the other coordinate).
std::vector<float> env_storage(const float* rgb, uint32_t n) {
    const int64_t m = (int64_t)n + 2, last = (int64_t)n - 1;
    std::vector<float> st((size_t)(m * m * 4));
    for (int64_t J = 0; J < m; ++J)
        for (int64_t I = 0; I < m; ++I) {
            int64_t i = I - 1, j = J - 1;
            if (i < 0 || i > last) {
                i = std::min(std::max<int64_t>(i, 0), last);
                j = last - j;
            }
            if (j < 0 || j > last) {
                i = last - i;
                j = std::min(std::max<int64_t>(j, 0), last);
            }
            const float* src = rgb + (size_t)(j * (int64_t)n + i) * 3;
            float* dst = st.data() + (size_t)(J * m + I) * 4;
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
            dst[3] = 0.0f;
        }
    return st;
}

}  // namespace

extern "C" {

int trhip_env_create(trhip_ctx* ctx, const float* rgb, uint32_t n, const float world_to_env[9], trhip_env** out) {
    // what needs no device first: the message tells which check fired even without a context
    if (!rgb || !world_to_env || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (n == 0 || n > kEnvMaxN) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_create: n must be in [1, %u], not %u", kEnvMaxN, n);
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(world_to_env[k])) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_create: world_to_env[%d] is not finite", k);
    float max_texel = 0.0f;
    for (size_t k = 0; k < (size_t)n * n * 3; ++k) {
        // the any-hit queue's contributions carry no poison bits: they must be finite, so the texels must be
        if (!std::isfinite(rgb[k]) || rgb[k] < 0.0f)
            return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_create: texel (%llu, %llu) channel %d is not finite or is negative", (unsigned long long)((k / 3) % n), (unsigned long long)((k / 3) / n), (int)(k % 3));
        max_texel = std::fmax(max_texel, rgb[k]);
    }
    if (!ctx) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<float> st = env_storage(rgb, n);
    std::unique_ptr<trhip_env> e(new trhip_env());
    e->ctx = ctx;
    e->n = n;
    e->max_texel = max_texel;
    std::memcpy(e->R, world_to_env, sizeof e->R);
    if (int rc = upload(ctx, e->tex, st.data(), st.size() * sizeof(float))) return rc;
    *out = e.release();
    return 0;
}

void trhip_env_free(trhip_env* env) {
    if (!env) return;
    (void)hipSetDevice(env->ctx->device);
    delete env;
}

int trhip_env_size(const trhip_env* env, uint32_t* n) {
    if (!env || !n) return fail(env ? env->ctx : nullptr, TRHIP_ERR_INVALID, "null argument");
    *n = env->n;
    return 0;
}

int trhip_env_eval(trhip_ctx* ctx, const trhip_env* env, const float* dirs3, uint64_t count, float* out_rgb3) {
    if (!ctx || !env || !dirs3 || !out_rgb3) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_eval: the environment belongs to another context");
    if (count == 0) return 0;
    if (count >= (1ull << 31)) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "trhip_env_eval: at most 2^31 - 1 directions per call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)count * 3 * sizeof(float);
    if (int rc = upload(ctx, ctx->scratch[0], dirs3, bytes)) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], bytes)) return rc;
    hipLaunchKernelGGL(k_env_eval, dim3(grid_for(ctx, count, 4)), dim3(kBlock), 0, ctx->stream, env->dev(), (const float*)ctx->scratch[0].p, count, (float*)ctx->scratch[1].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out_rgb3, ctx->scratch[1].p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
