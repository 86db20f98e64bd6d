// th_env.h — the environment map (include/tracehip.h, trhip_env; docs/design/25-sky.md): an octahedral map of n x n RGB texels and its deterministic bilinear lookup.
//
//   env_eval     direction -> radiance, the device function every environment term goes through
//   k_env_eval   count directions -> count radiances (trhip_env_eval: the lookup on its own)
//
// Storage: (n + 2) x (n + 2) float4 texels, texel (i, j) of the map at [(j + 1) * (n + 2) + (i + 1)], around them a one-texel gutter the host fills at creation with the
// octahedral edge wrap (tu_env.hip, env_storage): the lookup reads its four texels without a clamp and without a branch at the border.
// The octahedral map is plain arithmetic — no atan2, no acos — so the lookup is one Float32 operation per line under the numerics contract (no contraction, `/` correctly rounded).
#pragma once
#include "th_host.h"

namespace th {

struct DeviceEnv {
    const float4* tex;  // (n + 2)^2 texels with the gutter
    uint32_t n;
    float R[9];  // world_to_env, row-major: always multiplied, the identity included
};

TH_HD float env_sgn(float v) { return v < 0.0f ? -1.0f : 1.0f; }
TH_HD float env_lerp(float a, float b, float t) { return a + t * (b - a); }  // a == b returns a in every bit

// docs/design/25-sky.md "Lookup", line by line.
__device__ inline f3 env_eval(const DeviceEnv& env, f3 w) {
    const float ex = (env.R[0] * w.x + env.R[1] * w.y) + env.R[2] * w.z;
    const float ey = (env.R[3] * w.x + env.R[4] * w.y) + env.R[5] * w.z;
    const float ez = (env.R[6] * w.x + env.R[7] * w.y) + env.R[8] * w.z;
    const float s = (fabsf(ex) + fabsf(ey)) + fabsf(ez);
    if (!(s > 0.0f) || s == kInf) return mk3(0.0f, 0.0f, 0.0f);  // zero, NaN and Inf directions
    float px = ex / s, py = ey / s;
    if (ez < 0.0f) {
        const float qx = (1.0f - fabsf(py)) * env_sgn(px);
        const float qy = (1.0f - fabsf(px)) * env_sgn(py);
        px = qx;
        py = qy;
    }
    const float nf = (float)env.n;
    const float fx = (px * 0.5f + 0.5f) * nf - 0.5f;
    const float fy = (py * 0.5f + 0.5f) * nf - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    // [-1, n - 1] by construction; clamped as integers so that no rounding at px = +-1 can address outside the gutter
    const int last = (int)env.n - 1;
    const int ix = min(max((int)x0, -1), last), iy = min(max((int)y0, -1), last);
    const float4* row0 = env.tex + (size_t)(iy + 1) * (env.n + 2u) + (size_t)(ix + 1);
    const float4* row1 = row0 + (env.n + 2u);
    const float4 t00 = row0[0], t10 = row0[1], t01 = row1[0], t11 = row1[1];
    return mk3(env_lerp(env_lerp(t00.x, t10.x, tx), env_lerp(t01.x, t11.x, tx), ty), env_lerp(env_lerp(t00.y, t10.y, tx), env_lerp(t01.y, t11.y, tx), ty),
               env_lerp(env_lerp(t00.z, t10.z, tx), env_lerp(t01.z, t11.z, tx), ty));
}

template <int TH_ONE_COPY = 0>
__global__ __launch_bounds__(kBlock) void k_env_eval(DeviceEnv env, const float* __restrict__ dirs3, uint64_t count, float* __restrict__ out3) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock) {
        const f3 e = env_eval(env, mk3(dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]));
        out3[3 * i] = e.x;
        out3[3 * i + 1] = e.y;
        out3[3 * i + 2] = e.z;
    }
}

}  // namespace th

// The object behind the opaque handle: the map as the caller gave it is not kept, only its device storage.
struct trhip_env {
    trhip_ctx* ctx = nullptr;
    uint32_t n = 0;
    float R[9] = {};
    float max_texel = 0.0f;  // the largest channel of any texel: a frame refuses a scale that takes it to +Inf (tu_sky.hip)
    DevBuf tex;              // (n + 2)^2 float4
    DevBuf sampler;          // (n + 1)^2 floats once trhip_env_make_sampler has run: the marginal, then the conditionals (th_env_sample.h)
    DeviceEnv dev() const {
        DeviceEnv d{(const float4*)tex.p, n, {}};
        std::memcpy(d.R, R, sizeof R);
        return d;
    }
};
