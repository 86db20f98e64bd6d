// th_env_sample.h — importance sampling of the environment map (include/tracehip.h, trhip_env_make_sampler; docs/design/27-sky-importance.md): a piecewise-constant
// distribution over the n x n cells of the octahedral square, its deterministic sampler and its density.
//
//   env_sample     (u0, u1) -> direction (world space, unit length), distributed like the table
//   env_pdf        direction -> density with respect to solid angle, always evaluated from the direction
//   k_env_sample   count points -> count directions (trhip_env_sample: the sampler on its own)
//   k_env_pdf      count directions -> count densities (trhip_env_pdf)
//
// Tables (built on the host in Float64, tu_env_sample.hip, env_sampler_tables): the marginal m[0 .. n] over rows j, then one conditional c_j[0 .. n] per row: (n + 1)(n + 1) floats.
// Both functions are one Float32 operation per line under the numerics contract (no contraction, `/` and sqrt correctly rounded).
#pragma once
#include "th_env.h"

namespace th {

struct DeviceEnvSampler {
    const float* marg;  // m[0 .. n]
    const float* cond;  // c_j[0 .. n] of row j at cond + j (n + 1)
    uint32_t n;
};

constexpr float kEnvOneMinus = 0x1.fffffep-1f;  // 1 - 2^-24

// The largest k in [0, n - 1] with T[k] <= u, T[0] = 0 <= u: a fixed trip count of ceil(log2 n) steps, and for any table content no read outside T[0 .. n - 1].
__device__ inline uint32_t env_search(const float* __restrict__ T, uint32_t n, float u) {
    uint32_t lo = 0u;
    for (uint32_t step = n > 1u ? 1u << (31 - __clz((int)(n - 1u))) : 0u; step; step >>= 1) {
        const uint32_t k = lo + step;
        if (k <= n - 1u && T[k] <= u) lo = k;
    }
    return lo;
}

// docs/design/27-sky-importance.md "env_sample", line by line.
__device__ inline f3 env_sample(const DeviceEnvSampler& s, const float* R, float u0, float u1) {
    const float nf = (float)s.n;
    const uint32_t j = env_search(s.marg, s.n, u1);
    const float mj = s.marg[j];
    const float pj = s.marg[j + 1u] - mj;
    const float v = fminf((u1 - mj) / pj, kEnvOneMinus);
    const float* __restrict__ row = s.cond + (size_t)j * (s.n + 1u);
    const uint32_t i = env_search(row, s.n, u0);
    const float ci = row[i];
    const float pi = row[i + 1u] - ci;
    const float t = fminf((u0 - ci) / pi, kEnvOneMinus);
    const float qx = (((float)i + t) / nf) * 2.0f - 1.0f;
    const float qy = (((float)j + v) / nf) * 2.0f - 1.0f;
    const float a = fabsf(qx), b = fabsf(qy);
    const float ez = (1.0f - a) - b;
    float ex = qx, ey = qy;
    if (ez < 0.0f) {  // the inverse of the lookup's fold
        ex = (1.0f - b) * env_sgn(qx);
        ey = (1.0f - a) * env_sgn(qy);
    }
    // R^T: the matrix is orthonormal (trhip_env_make_sampler checks it)
    const f3 w = mk3((R[0] * ex + R[3] * ey) + R[6] * ez, (R[1] * ex + R[4] * ey) + R[7] * ez, (R[2] * ex + R[5] * ey) + R[8] * ez);
    const float l = norm(w);
    return w / l;
}

// docs/design/27-sky-importance.md "env_pdf", line by line.
__device__ inline float env_pdf(const DeviceEnvSampler& s, const float* R, f3 w) {
    const float ex = (R[0] * w.x + R[1] * w.y) + R[2] * w.z;
    const float ey = (R[3] * w.x + R[4] * w.y) + R[5] * w.z;
    const float ez = (R[6] * w.x + R[7] * w.y) + R[8] * w.z;
    const float sum = (fabsf(ex) + fabsf(ey)) + fabsf(ez);
    if (!(sum > 0.0f) || sum == kInf) return 0.0f;  // where env_eval returns zero
    float px = ex / sum, py = ey / sum;
    const float pz = ez / sum;
    const float r2 = (px * px + py * py) + pz * pz;  // before the fold: the point of the octahedron
    if (ez < 0.0f) {
        const float qx = (1.0f - fabsf(py)) * env_sgn(px);
        const float qy = (1.0f - fabsf(px)) * env_sgn(py);
        px = qx;
        py = qy;
    }
    const float nf = (float)s.n;
    const int last = (int)s.n - 1;
    const int i = min(max((int)floorf((px * 0.5f + 0.5f) * nf), 0), last);
    const int j = min(max((int)floorf((py * 0.5f + 0.5f) * nf), 0), last);
    const float* __restrict__ row = s.cond + (size_t)j * (s.n + 1u);
    const float pm = s.marg[j + 1] - s.marg[j];
    const float pc = row[i + 1] - row[i];
    return ((pm * pc) * ((nf * nf) * 0.25f)) * (r2 * sqrt_(r2));
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_env_sample(DeviceEnv env, DeviceEnvSampler smp, const float* __restrict__ u2, uint64_t count, float* __restrict__ out3) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock) {
        const f3 w = env_sample(smp, env.R, u2[2 * i], u2[2 * i + 1]);
        out3[3 * i] = w.x;
        out3[3 * i + 1] = w.y;
        out3[3 * i + 2] = w.z;
    }
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_env_pdf(DeviceEnv env, DeviceEnvSampler smp, const float* __restrict__ dirs3, uint64_t count, float* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock)
        out[i] = env_pdf(smp, env.R, mk3(dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]));
}

}  // namespace th

// the tables of an environment that has a sampler (trhip_env::sampler, th_env.h)
inline th::DeviceEnvSampler env_sampler_dev(const trhip_env* e) {
    const float* t = (const float*)e->sampler.p;
    return th::DeviceEnvSampler{t, t + (e->n + 1u), e->n};
}
