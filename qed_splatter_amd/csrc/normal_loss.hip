// Normal supervision in training: the loss on the rendered normal and the two per-Gaussian kernels of its backward pass.
// The accumulation itself is the unchanged compositing pair (composite.hip): qed_gaussian_normals writes a second set of
// records with the normal in the colour slots, qed_composite_fwd accumulates A = Sum_i alpha_i T_i n_i, and backwards a SECOND
// call of qed_composite_bwd with those records fills a second [C N, 16] accumulator (the "normal rows").  Around them:
//
//   qed_normal_loss           one streaming pass over the image.  n^ = A / |A| where alpha >= min_alpha and |A| > 1e-8
//                             (qed_normal_maps' rule), V = those pixels whose target is valid and whose mask is non-zero;
//                             per pixel l = mean_c |n^_c - g_c| (+ 1 - n^ . g with the cosine term).  Writes the UNSCALED
//                             d l / d A = (I - n^ n^T) / |A| (sign(n^ - g) / 3 - [cosine] g), zero outside V, and the
//                             workgroup's {count, Sum L1, Sum (1 - n^ . g)} as doubles; a one-workgroup launch folds them in
//                             a fixed order (qed_reduce.h): no floating-point atomics, the same input gives the same bits.
//                             The per-pixel arithmetic is double from the float32 inputs (|A| may be 1e-8: the gradient
//                             spans sixteen decades); the pass stays bound by its ~45 B per pixel (18 us at 1080p).
//   qed_gaussian_normals_bwd  one thread per Gaussian, looping over the cameras (no atomics): slots 8..10 of the normal rows
//                             are d L / d n_i in the camera frame; through n_i = +-R_v column k of R(q / |q|) -- the same k,
//                             sign and frame rules as qed_gaussian_normals, both piecewise constant -- to the RAW quaternion,
//                             normalisation Jacobian included.  A zero quaternion gets 0.  R_v itself is not differentiated.
//   qed_normal_rows_merge     one row per thread, 16-byte accesses: slots 0, 1 (2-D mean) and 4..7 (conic, opacity) of the
//                             normal rows, times a device scale, are added to the colour pass's rows in place; its slots
//                             2, 3 (absgrad), 8..10 (colour) and 11 (depth) keep their bits.  96 B per row (the first half of each).
#include "qed_common.h"

namespace qed {

constexpr int kNlCols = 3;                                    // count | sum of L1 over the channels | sum of 1 - n^ . g
constexpr int kNlMaxGrid = QED_NORMAL_LOSS_WS_DOUBLES / kNlCols;

__global__ void __launch_bounds__(256)
normal_loss_kernel(int n_pix, const float* __restrict__ accum, const float* __restrict__ alpha,
                   const float* __restrict__ target, const unsigned char* __restrict__ target_valid, unsigned valid_bits,
                   const float* __restrict__ mask, float min_alpha, int use_cosine, float* __restrict__ v_accum,
                   double* __restrict__ partials) {
    double acc[kNlCols] = {0.0, 0.0, 0.0};
    // kU pixels per trip, every load of the trip issued before the first use (clamped index, the pixel switched off by
    // `in`): the shape of normals.hip's angular-error pass
    constexpr int kU = 4;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < (size_t)n_pix; i0 += kU * stride) {
        float Av[kU][3], gv[kU][3], al[kU];
        bool ok[kU], in[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const size_t iu = i0 + u * stride;
            in[u] = iu < (size_t)n_pix;
            const size_t i = in[u] ? iu : i0;
            ok[u] = in[u] && (target_valid[i] & valid_bits) != 0 && (mask == nullptr || mask[i] != 0.f);
            al[u] = alpha[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) { Av[u][k] = accum[3 * i + k]; gv[u][k] = target[3 * i + k]; }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {                        // (in index order: the sums' order is fixed)
            if (!in[u]) continue;
            const size_t i = i0 + u * stride;
            float vA[3] = {0.f, 0.f, 0.f};
            const double A0 = Av[u][0], A1 = Av[u][1], A2 = Av[u][2];
            const double len = sqrt(A0 * A0 + A1 * A1 + A2 * A2);
            if (ok[u] && al[u] >= min_alpha && len > 1e-8) {
                const double il = 1.0 / len;
                const double n[3] = {A0 * il, A1 * il, A2 * il};
                const double g[3] = {(double)gv[u][0], (double)gv[u][1], (double)gv[u][2]};
                double l1 = 0.0, dot = 0.0, vn[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double d = n[k] - g[k];
                    l1 += fabs(d);
                    dot += n[k] * g[k];
                    vn[k] = (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)) * (1.0 / 3.0) - (use_cosine ? g[k] : 0.0);
                }
                const double nv = n[0] * vn[0] + n[1] * vn[1] + n[2] * vn[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) vA[k] = (float)((vn[k] - n[k] * nv) * il);
                acc[0] += 1.0;
                acc[1] += l1;
                acc[2] += 1.0 - dot;
            }
            v_accum[3 * i] = vA[0]; v_accum[3 * i + 1] = vA[1]; v_accum[3 * i + 2] = vA[2];
        }
    }
    __shared__ double s_w[kNlCols][4];
    __shared__ double s[kNlCols];
    block_sum_d(acc, s_w, s);
    if (threadIdx.x < kNlCols) partials[(size_t)threadIdx.x * kNlMaxGrid + blockIdx.x] = s[threadIdx.x];
}

__global__ void __launch_bounds__(256)
normal_loss_finalize_kernel(int n_blocks, const double* __restrict__ partials, double normal_lambda, int use_cosine,
                            double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kNlCols][4];
    __shared__ double s[kNlCols];
    double v[kNlCols] = {0.0, 0.0, 0.0};
    for (int blk = threadIdx.x; blk < n_blocks; blk += 256) {
#pragma unroll
        for (int c = 0; c < kNlCols; ++c) v[c] += partials[(size_t)c * kNlMaxGrid + blk];
    }
    block_sum_d(v, s_w, s);
    if (threadIdx.x == 0) {
        const double count = s[0];
        const double div = count > 0.0 ? count : 1.0;         // (an empty V: every sum is 0, and so is the loss)
        const double l1 = s[1] / (3.0 * div);
        const double cosine = use_cosine ? s[2] / div : 0.0;
        const double loss = normal_lambda * (l1 + cosine);
        out[0] = loss; out[1] = l1; out[2] = cosine; out[3] = count;
        if (out_f != nullptr) { out_f[0] = (float)loss; out_f[1] = (float)(normal_lambda / div); }
    }
}

// ---- d L / d n_i -> d L / d (raw quaternion) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
gaussian_normals_bwd_kernel(int N, int C, const float* __restrict__ means, const float* __restrict__ quats,
                            const float* __restrict__ scales, const float* __restrict__ viewmats,
                            const int* __restrict__ radii, const float4* __restrict__ rows, const float* __restrict__ scale,
                            int add, float* __restrict__ v_quats) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float s0 = scales[3 * n], s1 = scales[3 * n + 1], s2 = scales[3 * n + 2];
    // (quats / v_quats sit at float offset 6 N of the flat layout: 8-byte aligned only, so no 16-byte access)
    const float w = quats[4 * n], x = quats[4 * n + 1], y = quats[4 * n + 2], z = quats[4 * n + 3];
    const float m[3] = {means[3 * n], means[3 * n + 1], means[3 * n + 2]};

    int k = 0;                                                // qed_gaussian_normals' rule: strict <, the lowest index wins
    float smin = s0;
    if (s1 < smin) { k = 1; smin = s1; }
    if (s2 < smin) k = 2;

    const float n2 = w * w + x * x + y * y + z * z;
    const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
    const float unit = n2 > 0.f ? 1.f : 0.f;
    const float qw = w * inv, qx = x * inv, qy = y * inv, qz = z * inv;
    float nw[3];                                              // column k of R(q / |q|), as the forward kernel forms it
    if (k == 0) {
        nw[0] = unit - 2.f * (qy * qy + qz * qz); nw[1] = 2.f * (qx * qy + qw * qz); nw[2] = 2.f * (qx * qz - qw * qy);
    } else if (k == 1) {
        nw[0] = 2.f * (qx * qy - qw * qz); nw[1] = unit - 2.f * (qx * qx + qz * qz); nw[2] = 2.f * (qy * qz + qw * qx);
    } else {
        nw[0] = 2.f * (qx * qz + qw * qy); nw[1] = 2.f * (qy * qz - qw * qx); nw[2] = unit - 2.f * (qx * qx + qy * qy);
    }

    float v[3] = {0.f, 0.f, 0.f};                             // d L / d (column k), world frame, summed over the cameras
    for (int c = 0; c < C; ++c) {
        const size_t slot = (size_t)c * N + n;
        if (radii != nullptr && radii[slot] <= 0) continue;   // a culled slot contributes nothing
        const float4 g4 = rows[4 * slot + 2];                 // row slots 8..11: d L / d n_i in the camera frame | depth
        const float* V = viewmats + 16 * (size_t)c;
        const float R[9] = {V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
        const float t[3] = {V[3], V[7], V[11]};
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float o = -(R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]);
            d += nw[j] * (m[j] - o);
        }
        const float sgn = d > 0.f ? -1.f : 1.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += sgn * (R[j] * g4.x + R[3 + j] * g4.y + R[6 + j] * g4.z);    // R_v^T
    }

    float gq[4];                                              // d L / d (unit quaternion) = (d column k / d q^)^T v
    if (k == 0) {
        gq[0] = 2.f * (qz * v[1] - qy * v[2]);
        gq[1] = 2.f * (qy * v[1] + qz * v[2]);
        gq[2] = -4.f * qy * v[0] + 2.f * (qx * v[1] - qw * v[2]);
        gq[3] = -4.f * qz * v[0] + 2.f * (qw * v[1] + qx * v[2]);
    } else if (k == 1) {
        gq[0] = 2.f * (qx * v[2] - qz * v[0]);
        gq[1] = 2.f * qy * v[0] - 4.f * qx * v[1] + 2.f * qw * v[2];
        gq[2] = 2.f * (qx * v[0] + qz * v[2]);
        gq[3] = -2.f * qw * v[0] - 4.f * qz * v[1] + 2.f * qy * v[2];
    } else {
        gq[0] = 2.f * (qy * v[0] - qx * v[1]);
        gq[1] = 2.f * qz * v[0] - 2.f * qw * v[1] - 4.f * qx * v[2];
        gq[2] = 2.f * qw * v[0] + 2.f * qz * v[1] - 4.f * qy * v[2];
        gq[3] = 2.f * (qx * v[0] + qy * v[1]);
    }
    // q^ = q / |q|: d L / d q = (g - q^ (q^ . g)) / |q|; inv = 0 for the zero quaternion, whose gradient is 0
    const float qg = qw * gq[0] + qx * gq[1] + qy * gq[2] + qz * gq[3];
    const float sc = (scale != nullptr ? scale[0] : 1.f) * inv;
    float out[4] = {(gq[0] - qw * qg) * sc, (gq[1] - qx * qg) * sc, (gq[2] - qy * qg) * sc, (gq[3] - qz * qg) * sc};
#pragma unroll
    for (int j = 0; j < 4; ++j) v_quats[4 * n + j] = add ? v_quats[4 * n + j] + out[j] : out[j];
}

// ---- the normal rows into the colour pass's rows -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
normal_rows_merge_kernel(long long total, const float4* __restrict__ normal_rows, const float* __restrict__ scale,
                         float4* __restrict__ rows) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= total) return;
    const float4 a0 = normal_rows[4 * r], a1 = normal_rows[4 * r + 1];
    float4 d0 = rows[4 * r], d1 = rows[4 * r + 1];
    const float s = scale != nullptr ? scale[0] : 1.f;
    d0.x += s * a0.x; d0.y += s * a0.y;                       // 2-D mean; slots 2, 3 (absgrad) are written back as read
    d1.x += s * a1.x; d1.y += s * a1.y; d1.z += s * a1.z; d1.w += s * a1.w;      // conic a, b, c | opacity
    rows[4 * r] = d0;
    rows[4 * r + 1] = d1;
}

}  // namespace qed

using namespace qed;

extern "C" int qed_normal_loss(int32_t n_pix, const float* accum, const float* alpha, const float* target,
                               const uint8_t* target_valid, uint32_t valid_bits, const float* mask, float min_alpha,
                               int32_t use_cosine, float normal_lambda, double* workspace, float* v_accum, double* out,
                               float* out_f, void* stream) {
    QED_REQUIRE(n_pix >= 0, "negative size");
    QED_REQUIRE(workspace && out, "null pointer");
    QED_REQUIRE(n_pix == 0 || (accum && alpha && target && target_valid && v_accum), "null input");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "misaligned double pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = n_pix == 0 ? 0u : stream_grid(n_pix, kNlMaxGrid);
    if (grid > 0)
        hipLaunchKernelGGL(normal_loss_kernel, dim3(grid), dim3(256), 0, st, n_pix, accum, alpha, target, target_valid,
                           valid_bits, mask, min_alpha, use_cosine ? 1 : 0, v_accum, workspace);
    hipLaunchKernelGGL(normal_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (int)grid, (const double*)workspace,
                       (double)normal_lambda, use_cosine ? 1 : 0, out, out_f);
    return check_launch("qed_normal_loss");
}

extern "C" int qed_gaussian_normals_bwd(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                                        const float* viewmats, const int32_t* radii, const float* normal_rows,
                                        const float* scale, uint32_t flags, int32_t add, float* v_quats, void* stream) {
    (void)flags;                                              // QED_F_LOG_SCALES: the order of the logarithms is the scales'
    QED_REQUIRE(N >= 0 && C >= 0, "negative size");
    if (N == 0) return QED_OK;
    QED_REQUIRE(v_quats && quats, "null pointer");
    QED_REQUIRE(C == 0 || (means && scales && viewmats && normal_rows), "null input");
    QED_REQUIRE(((uintptr_t)normal_rows & 15) == 0, "rows must be 16-byte aligned");
    const long long grid = ((long long)N + 255) / 256;
    hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, N, C, means,
                       quats, scales, viewmats, radii, (const float4*)normal_rows, scale, add ? 1 : 0, v_quats);
    return check_launch("qed_gaussian_normals_bwd");
}

extern "C" int qed_normal_rows_merge(int64_t total, const float* normal_rows, const float* scale, float* rows,
                                     void* stream) {
    QED_REQUIRE(total >= 0, "negative size");
    if (total == 0) return QED_OK;
    QED_REQUIRE(normal_rows && rows, "null pointer");
    QED_REQUIRE((((uintptr_t)normal_rows | (uintptr_t)rows) & 15) == 0, "rows must be 16-byte aligned");
    const long long grid = ((long long)total + 255) / 256;
    QED_REQUIRE(grid <= 0x7fffffffLL, "too many rows");
    hipLaunchKernelGGL(normal_rows_merge_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (long long)total,
                       (const float4*)normal_rows, scale, (float4*)rows);
    return check_launch("qed_normal_rows_merge");
}
