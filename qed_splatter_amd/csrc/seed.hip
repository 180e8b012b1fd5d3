// Seeding the Gaussians from a point cloud: splatfacto's populate_modules on the distances of qed_knn_query
// (self-query, k = 3, QED_KNN_SKIP_FIRST = k_nearest_sklearn's [:, 1:]).  One streaming launch writes five of the six
// parameter groups of the model's flat buffer per row and zeroes the sixth; the means are the points themselves and are
// copied by the caller.  Nothing is concatenated.
//
//   scales        logf(max(mean_j dist[n, j], min_distance)) in all three columns; the mean is an fp32 sum in column order
//                 divided by k.  Upstream has no clamp: three coincident points give log 0 = -inf there, and here with
//                 min_distance = 0.  status[0] counts the clamped rows (integer atomics: exact in any order).
//   quats         random_quat_tensor: (sqrt(1-u) sin 2 pi v, sqrt(1-u) cos 2 pi v, sqrt(u) sin 2 pi w, sqrt(u) cos 2 pi w),
//                 u, v, w = the top 24 bits of rng64(seed, 0, row, stream) / 2^24 in [0, 1): a function of (seed, row)
//   opacities     logit(0.1)
//   features_dc   with colours: RGB2SH(c / 255) for sh_coeffs > 1, logit(c / 255, eps = 1e-10) for sh_coeffs == 1, both
//                 evaluated in float64 and rounded once (the byte 255 gives +23.03 in colour-only mode, where an fp32
//                 evaluation of the clamp 1 - 1e-10 = 1 would give +inf); without colours: uniform [0, 1)
//   features_rest 0
#include "qed_common.h"

#include <math.h>

namespace qed {

constexpr int kSeedThreads = 256;

__device__ __forceinline__ float seed_uniform(unsigned long long seed, unsigned long long index, unsigned stream) {
    return (float)(rng64(seed, 0ull, index, stream) >> 40) * (1.0f / 16777216.0f);     // 24 bits: exact, < 1
}

__global__ void __launch_bounds__(kSeedThreads)
seed_gaussians_kernel(int n, const float* __restrict__ dist, int k, const unsigned char* __restrict__ colors, int sh_coeffs,
                      unsigned long long seed, float min_distance, float* __restrict__ scales, float* __restrict__ quats,
                      float* __restrict__ opacities, float* __restrict__ features_dc, float* __restrict__ features_rest,
                      int* __restrict__ status) {
    int clamped = 0;
    const float inv_k = 1.0f / (float)k;
    for (long long i = (long long)blockIdx.x * kSeedThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSeedThreads) {
        float sum = 0.f;
        for (int j = 0; j < k; ++j) sum += dist[i * k + j];
        const float mean = sum * inv_k;
        clamped += mean < min_distance ? 1 : 0;
        const float s = logf(fmaxf(mean, min_distance));
        scales[3 * i] = s; scales[3 * i + 1] = s; scales[3 * i + 2] = s;
        const float u = seed_uniform(seed, (unsigned long long)i, kRngSeedQuatU);
        const float v = seed_uniform(seed, (unsigned long long)i, kRngSeedQuatV);
        const float w = seed_uniform(seed, (unsigned long long)i, kRngSeedQuatW);
        const float a = sqrtf(1.f - u), b = sqrtf(u);
        float sv, cv, sw, cw;
        sincospif(2.f * v, &sv, &cv);
        sincospif(2.f * w, &sw, &cw);
        quats[4 * i] = a * sv; quats[4 * i + 1] = a * cv; quats[4 * i + 2] = b * sw; quats[4 * i + 3] = b * cw;
        opacities[i] = -2.1972245773362196f;                                   // log(0.1 / 0.9)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float f;
            if (colors != nullptr) {
                const double x = (double)colors[3 * i + ch] / 255.0;
                if (sh_coeffs > 1) {
                    f = (float)((x - 0.5) / 0.28209479177387814);
                } else {
                    const double y = fmin(fmax(x, 1e-10), 1.0 - 1e-10);
                    f = (float)log(y / (1.0 - y));
                }
            } else {
                f = seed_uniform(seed, (unsigned long long)(3 * i + ch), kRngSeedColor);
            }
            features_dc[3 * i + ch] = f;
        }
    }
    const long long n_rest = (long long)n * (sh_coeffs - 1) * 3;
    for (long long i = (long long)blockIdx.x * kSeedThreads + threadIdx.x; i < n_rest; i += (long long)gridDim.x * kSeedThreads)
        features_rest[i] = 0.f;
    clamped = wave_sum_i(clamped);
    if ((threadIdx.x & 63) == 0 && clamped) atomicAdd(&status[0], clamped);
}

// splatfacto's random initialisation: (rand(n, 3) - 0.5) * scale
__global__ void __launch_bounds__(kSeedThreads)
seed_random_points_kernel(long long n3, unsigned long long seed, float scale, float* __restrict__ points) {
    for (long long i = (long long)blockIdx.x * kSeedThreads + threadIdx.x; i < n3; i += (long long)gridDim.x * kSeedThreads)
        points[i] = (seed_uniform(seed, (unsigned long long)i, kRngSeedPoint) - 0.5f) * scale;
}

}  // namespace qed

using namespace qed;

extern "C" int qed_seed_gaussians(int32_t n, const float* dist, int32_t k, const uint8_t* colors_u8, int32_t sh_coeffs,
                                  uint64_t seed, float min_distance, int32_t flags, float* scales, float* quats,
                                  float* opacities, float* features_dc, float* features_rest, int32_t* status,
                                  void* stream) {
    QED_REQUIRE(n >= 0 && n < (1 << 30), "n out of range");
    QED_REQUIRE(k >= 1 && k <= 8, "k must be in [1, 8]");
    QED_REQUIRE(sh_coeffs >= 1 && sh_coeffs <= 16, "sh_coeffs must be in [1, 16]");
    QED_REQUIRE(min_distance >= 0.f && isfinite(min_distance), "min_distance must be finite and >= 0");
    QED_REQUIRE(flags == 0, "unknown flags");
    QED_REQUIRE(status, "null buffers (status)");
    if (n > 0)
        QED_REQUIRE(dist && scales && quats && opacities && features_dc && (features_rest || sh_coeffs == 1), "null buffers");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * QED_STATUS_WORDS, st) != hipSuccess) {
        set_error("qed_seed_gaussians: memset failed");
        return QED_E_LAUNCH;
    }
    if (n == 0) return QED_OK;
    hipLaunchKernelGGL(seed_gaussians_kernel, dim3(stream_grid(n)), dim3(kSeedThreads), 0, st, n, dist, k,
                       (const unsigned char*)colors_u8, sh_coeffs, (unsigned long long)seed, min_distance, scales, quats,
                       opacities, features_dc, features_rest, status);
    return check_launch("qed_seed_gaussians");
}

extern "C" int qed_seed_random_points(int32_t n, uint64_t seed, float scale, float* points, void* stream) {
    QED_REQUIRE(n >= 0 && n < (1 << 30), "n out of range");
    QED_REQUIRE(isfinite(scale), "scale must be finite");
    if (n == 0) return QED_OK;
    QED_REQUIRE(points, "null buffers");
    hipLaunchKernelGGL(seed_random_points_kernel, dim3(stream_grid(3ll * n)), dim3(kSeedThreads), 0, (hipStream_t)stream,
                       3ll * n, (unsigned long long)seed, scale, points);
    return check_launch("qed_seed_random_points");
}
