// tu_env_sample.hip — the sampling distribution of an environment map (trhip_env_make_sampler / trhip_env_sample / trhip_env_pdf; th_env_sample.h,
// docs/design/27-sky-importance.md): the checks, the tables — built here on the host in Float64, from the gutter storage tu_env.hip made, in the order the specification
// gives —, the upload, and the sampler and the density on their own.
#include "th_env_sample.h"

#include <cmath>

namespace {

// (n + 1)(n + 1) floats: the marginal m[0 .. n], then the conditional c_j[0 .. n] of every row j.  `st` is the gutter storage, (n + 2)^2 float4.  Empty: every weight is zero.
// The order of every sum is the specification's, and tests/sky_is_model.py's.
std::vector<float> env_sampler_tables(const std::vector<float>& st, uint32_t n) {
    const size_t m = (size_t)n + 2, n1 = (size_t)n + 1;
    std::vector<double> y(m * m);
    for (size_t k = 0; k < m * m; ++k) y[k] = ((double)st[4 * k] + (double)st[4 * k + 1]) + (double)st[4 * k + 2];
    const double kern[3] = {0.125, 0.75, 0.125};  // the integral of the bilinear tent over a cell
    // the Jacobian of a cell's centre, d(omega) / d(area of the square) = 1 / |P|^3 with P the centre's point of the octahedron: a function of one coordinate pair
    auto centre = [n](size_t i) { return std::fabs(((double)i + 0.5) / (double)n * 2.0 - 1.0); };
    std::vector<double> w((size_t)n * n);
    for (size_t j = 0; j < n; ++j)
        for (size_t i = 0; i < n; ++i) {
            double W = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) W += (kern[a] * kern[b]) * y[(j + (size_t)b) * m + (i + (size_t)a)];  // y(i + a - 1, j + b - 1) of the map is storage (i + a, j + b)
            const double ca = centre(i), cb = centre(j);
            double px, py, pz;
            if (ca + cb <= 1.0) {
                px = ca, py = cb, pz = (1.0 - ca) - cb;
            } else {
                px = 1.0 - cb, py = 1.0 - ca, pz = (ca + cb) - 1.0;
            }
            const double r2 = (px * px + py * py) + pz * pz;
            w[j * n + i] = W * (1.0 / (r2 * std::sqrt(r2)));
        }
    std::vector<double> rows(n);
    double total = 0.0;
    for (size_t j = 0; j < n; ++j) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r += w[j * n + i];
        rows[j] = r;
        total += r;
    }
    if (!(total > 0.0)) return {};
    std::vector<float> t(n1 * n1);
    double acc = 0.0;
    for (size_t j = 0; j < n; ++j) {
        t[j] = (float)(acc / total);
        acc += rows[j];
        float* c = t.data() + n1 * (j + 1);
        double ca = 0.0;
        for (size_t i = 0; i < n; ++i) {
            c[i] = rows[j] > 0.0 ? (float)(ca / rows[j]) : (float)((double)i / (double)n);  // a row without weight is never selected: its marginal step is 0
            ca += w[j * n + i];
        }
        c[n] = 1.0f;
    }
    t[n] = 1.0f;
    return t;
}

int sampler_call_checks(trhip_ctx* ctx, const trhip_env* env, const void* in, const void* out, uint64_t count, const char* who) {
    if (!ctx || !env || !in || !out) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "%s: the environment belongs to another context", who);
    if (!env->sampler.p) return fail(ctx, TRHIP_ERR_INVALID, "%s: the environment has no sampler (trhip_env_make_sampler)", who);
    if (count >= (1ull << 31)) return fail(ctx, TRHIP_ERR_UNSUPPORTED, "%s: at most 2^31 - 1 entries per call", who);
    return 0;
}

}  // namespace

extern "C" {

int trhip_env_make_sampler(trhip_ctx* ctx, trhip_env* env) {
    if (!ctx || !env) return fail(ctx, TRHIP_ERR_INVALID, "null argument");
    if (env->ctx != ctx) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_make_sampler: the environment belongs to another context");
    if (env->sampler.p) return 0;  // idempotent: the map never changes
    // sampling needs R^-1 = R^T and a density the matrix preserves
    double worst = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)env->R[3 * r + k] * (double)env->R[3 * c + k];
            worst = std::fmax(worst, std::fabs(d - (r == c ? 1.0 : 0.0)));
        }
    if (!(worst <= 1e-5)) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_make_sampler: world_to_env is not orthonormal (max |R R^T - I| = %g > 1e-5)", worst);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)env->n + 2;
    std::vector<float> st(m * m * 4);
    HIP_TRY(ctx, hipMemcpy(st.data(), env->tex.p, st.size() * sizeof(float), hipMemcpyDeviceToHost));
    const std::vector<float> t = env_sampler_tables(st, env->n);
    if (t.empty()) return fail(ctx, TRHIP_ERR_INVALID, "trhip_env_make_sampler: every weight of the map is zero: there is nothing to sample");
    return upload(ctx, env->sampler, t.data(), t.size() * sizeof(float));
}

int trhip_env_sample(trhip_ctx* ctx, const trhip_env* env, const float* u2, uint64_t count, float* out_dir3) {
    if (int rc = sampler_call_checks(ctx, env, u2, out_dir3, count, "trhip_env_sample")) return rc;
    if (count == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)count * 3 * sizeof(float);
    if (int rc = upload(ctx, ctx->scratch[0], u2, (size_t)count * 2 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], bytes)) return rc;
    hipLaunchKernelGGL(k_env_sample, dim3(grid_for(ctx, count, 4)), dim3(kBlock), 0, ctx->stream, env->dev(), env_sampler_dev(env), (const float*)ctx->scratch[0].p, count,
                       (float*)ctx->scratch[1].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out_dir3, ctx->scratch[1].p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int trhip_env_pdf(trhip_ctx* ctx, const trhip_env* env, const float* dirs3, uint64_t count, float* out_pdf) {
    if (int rc = sampler_call_checks(ctx, env, dirs3, out_pdf, count, "trhip_env_pdf")) return rc;
    if (count == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)count * sizeof(float);
    if (int rc = upload(ctx, ctx->scratch[0], dirs3, (size_t)count * 3 * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->scratch[1], bytes)) return rc;
    hipLaunchKernelGGL(k_env_pdf, dim3(grid_for(ctx, count, 4)), dim3(kBlock), 0, ctx->stream, env->dev(), env_sampler_dev(env), (const float*)ctx->scratch[0].p, count,
                       (float*)ctx->scratch[1].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out_pdf, ctx->scratch[1].p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
