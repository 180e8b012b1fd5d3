// Camera pose optimiser, Nerfstudio's CameraOptimizer in mode SO3xR3 (qed_splat.h: qed_pose_apply, qed_pose_apply_bwd,
// qed_pose_step).  pose_adjustment[n_rows, 6] = (d, w) per training camera: translation d, rotation vector w.
//
//   a = sqrt(max(|w|^2, 1e-4));  R(w) = I + (sin a / a) K + ((1 - cos a) / a^2) K^2,  K = skew(w)
//   c2w_opt = c2w [[R, d], [0, 0, 0, 1]]  i.e.  R_opt = R0 R,  t_opt = R0 d + t0
//
// Below the clamp (|w| < 0.01) the angle is held at 0.01 and passes no gradient: R is then only approximately a rotation,
// as upstream.  The kernels are latency-bound (a few thousand rows at most): what counts is that a training step takes ONE
// launch for the pose it renders with and ONE for everything after the projection backward.
#include "qed_common.h"

namespace qed {

constexpr float kPoseClamp = 1e-4f;          // the clamp on |w|^2

struct PoseCoef {
    float A, B;             // sin a / a, (1 - cos a) / a^2
    float a;
    bool free_angle;        // |w|^2 >= the clamp: a follows w
};

__device__ __forceinline__ PoseCoef pose_coef(const float* __restrict__ w) {
    PoseCoef c;
    const float n2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    c.free_angle = n2 >= kPoseClamp;
    c.a = sqrtf(fmaxf(n2, kPoseClamp));
    const float ia = 1.f / c.a;
    c.A = sinf(c.a) * ia;
    // 1 - cos a = 2 sin^2(a / 2): no cancellation at small angles (1 - cosf(0.01) keeps three digits)
    const float h = sinf(0.5f * c.a) * ia;
    c.B = 2.f * h * h;
    return c;
}

// K = skew(w) and K^2 = w w^T - |w|^2 I, row-major
__device__ __forceinline__ void pose_skew(const float* __restrict__ w, float* K, float* K2) {
    K[0] = 0.f;   K[1] = -w[2]; K[2] = w[1];
    K[3] = w[2];  K[4] = 0.f;   K[5] = -w[0];
    K[6] = -w[1]; K[7] = w[0];  K[8] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
}

// out[3,4] = c2w[3,4] [[R(w), d], [0 0 0 1]] for the row t = (d, w)
__device__ __forceinline__ void pose_compose(const float* __restrict__ t, const float* __restrict__ c2w, float* out) {
    const PoseCoef c = pose_coef(t + 3);
    float K[9], K2[9], R[9];
    pose_skew(t + 3, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.f : 0.f) + c.A * K[i] + c.B * K2[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r0 = c2w[4 * i], r1 = c2w[4 * i + 1], r2 = c2w[4 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) out[4 * i + j] = r0 * R[j] + r1 * R[3 + j] + r2 * R[6 + j];
        out[4 * i + 3] = r0 * t[0] + r1 * t[1] + r2 * t[2] + c2w[4 * i + 3];
    }
}

// g[6] = the gradient of the row t for an upstream gradient v[3,4] of pose_compose's result
__device__ __forceinline__ void pose_compose_bwd(const float* __restrict__ t, const float* __restrict__ c2w,
                                                 const float* __restrict__ v, float* g) {
    const float* w = t + 3;
    const PoseCoef c = pose_coef(w);
    float K[9], K2[9], vR[9];
    pose_skew(w, K, K2);
    // R_opt = R0 R, t_opt = R0 d + t0:  v_R = R0^T v_Ropt,  v_d = R0^T v_topt
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) vR[3 * a + b] = c2w[a] * v[b] + c2w[4 + a] * v[4 + b] + c2w[8 + a] * v[8 + b];
        g[a] = c2w[a] * v[3] + c2w[4 + a] * v[7] + c2w[8 + a] * v[11];
    }
    // R = I + A K + B K K:  v_K = A v_R + B (v_R K^T + K^T v_R),  v_A = <v_R, K>,  v_B = <v_R, K K>
    float vK[9];
    float vA = 0.f, vB = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += vR[3 * i + k] * K[3 * j + k] + K[3 * k + i] * vR[3 * k + j];
            vK[3 * i + j] = c.A * vR[3 * i + j] + c.B * s;
            vA += vR[3 * i + j] * K[3 * i + j];
            vB += vR[3 * i + j] * K2[3 * i + j];
        }
    g[3] = vK[7] - vK[5];
    g[4] = vK[2] - vK[6];
    g[5] = vK[3] - vK[1];
    if (c.free_angle) {
        // dA/da = (a cos a - sin a) / a^2,  dB/da = (a sin a - 2 (1 - cos a)) / a^3: both cancel at small angles, where
        // their series (-a/3 + a^3/30 - a^5/840 + a^7/45360, -a/12 + a^3/180 - a^5/6720 + a^7/453600) are exact to float
        const float a = c.a, a2 = a * a;
        float dA, dB;
        if (a < 0.5f) {
            dA = a * (-1.f / 3.f + a2 * (1.f / 30.f + a2 * (-1.f / 840.f + a2 * (1.f / 45360.f))));
            dB = a * (-1.f / 12.f + a2 * (1.f / 180.f + a2 * (-1.f / 6720.f + a2 * (1.f / 453600.f))));
        } else {
            const float s = sinf(a), h = sinf(0.5f * a);
            dA = (a * cosf(a) - s) / a2;
            dB = (a * s - 4.f * h * h) / (a2 * a);
        }
        const float va = (vA * dA + vB * dB) / a;          // a = |w|:  da/dw = w / a
        g[3] += va * w[0];
        g[4] += va * w[1];
        g[5] += va * w[2];
    }
}

// The gradient of c2w[3,4] for the gradient G = v_viewmats[4,4] of the view matrix get_viewmat (model.py:22-38) makes of
// it: Rf = R * (1, -1, -1) by columns, viewmat = [[Rf^T, -Rf^T t], [0 0 0 1]].  G is the gradient of a GENERAL matrix (see
// qed_project_bwd on campos), so this is the plain chain rule of those statements, which is what autograd does.
__device__ __forceinline__ void viewmat_bwd(const float* __restrict__ c2w, const float* __restrict__ G, float* v) {
    const float f[3] = {1.f, -1.f, -1.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float vt = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            v[4 * i + j] = f[j] * (G[4 * j + i] - G[4 * j + 3] * c2w[4 * i + 3]);
            vt -= c2w[4 * i + j] * f[j] * G[4 * j + 3];
        }
        v[4 * i + 3] = vt;
    }
}

// camera c of the launch -> its row; -1 when the index is out of range (the outputs are then NaN, nothing is read)
__device__ __forceinline__ int pose_row_of(const int32_t* __restrict__ rows, int row0, int c, int n_rows) {
    const int r = rows != nullptr ? rows[c] : row0 + c;
    return (r >= 0 && r < n_rows) ? r : -1;
}

// sum over all rows of |d| and of |w| by ONE workgroup of 256 threads; every thread must call.  s[0], s[1] afterwards.
__device__ __forceinline__ void pose_norm_sums(const float* __restrict__ pose, int n_rows, double (*s_w)[4], double* s) {
    float acc[2] = {0.f, 0.f};
    for (int r = threadIdx.x; r < n_rows; r += 256) {
        const float* t = pose + 6 * (size_t)r;
        acc[0] += sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        acc[1] += sqrtf(t[3] * t[3] + t[4] * t[4] + t[5] * t[5]);
    }
    block_sum_f<2, 256>(acc, s_w, s);
}

__global__ void __launch_bounds__(256)
pose_apply_kernel(int C, int n_rows, const float* __restrict__ pose, const int32_t* __restrict__ rows, int row0,
                  const float* __restrict__ c2w_in, float* __restrict__ c2w_out, float trans_pen, float rot_pen,
                  float* __restrict__ reg_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        const int r = pose_row_of(rows, row0, c, n_rows);
        float in[12], out[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) in[i] = c2w_in[12 * (size_t)c + i];
        if (r >= 0) {
            float t[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) t[i] = pose[6 * (size_t)r + i];
            pose_compose(t, in, out);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) out[i] = __builtin_nanf("");
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) c2w_out[12 * (size_t)c + i] = out[i];
    }
    if (reg_out != nullptr && blockIdx.x == 0) {               // (uniform over the workgroup)
        __shared__ double s_w[2][4];
        __shared__ double s[2];
        pose_norm_sums(pose, n_rows, s_w, s);
        if (threadIdx.x == 0) reg_out[0] = (float)(((double)trans_pen * s[0] + (double)rot_pen * s[1]) / (double)n_rows);
    }
}

__global__ void __launch_bounds__(256)
pose_apply_bwd_kernel(int C, int n_rows, const float* __restrict__ pose, const int32_t* __restrict__ rows, int row0,
                      const float* __restrict__ c2w_in, const float* __restrict__ v_c2w, float* __restrict__ v_rows) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int r = pose_row_of(rows, row0, c, n_rows);
    float g[6];
    if (r >= 0) {
        float t[6], in[12], v[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) t[i] = pose[6 * (size_t)r + i];
#pragma unroll
        for (int i = 0; i < 12; ++i) { in[i] = c2w_in[12 * (size_t)c + i]; v[i] = v_c2w[12 * (size_t)c + i]; }
        pose_compose_bwd(t, in, v, g);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = __builtin_nanf("");
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) v_rows[6 * (size_t)c + i] = g[i];
}

// torch.optim.Adam's update as adam.hip's adam_update writes it (omb = 1 - beta formed in double on the host)
struct PoseAdam {
    float beta1, beta2, omb1, omb2, eps, inv_bc1, inv_bc2_sqrt, lr;
};

// ONE workgroup.  The thread that owns the step's row turns v_viewmats into that row's gradient and zeroes the buffer
// (nobody else touches it); every thread adds the regulariser's gradient to its rows and takes their Adam step.
__global__ void __launch_bounds__(256)
pose_step_kernel(int n_rows, int row, float* __restrict__ pose, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                 const float* __restrict__ c2w_in, float* __restrict__ v_viewmats, float trans_pen, float rot_pen,
                 PoseAdam co, float* __restrict__ raw_grad, float* __restrict__ reg_out, const int* __restrict__ skip) {
    __shared__ double s_w[2][4];
    __shared__ double s[2];
    const bool skipped = skip != nullptr && skip[0] != 0;
    if (reg_out != nullptr) {
        pose_norm_sums(pose, n_rows, s_w, s);
        if (threadIdx.x == 0) reg_out[0] = (float)(((double)trans_pen * s[0] + (double)rot_pen * s[1]) / (double)n_rows);
    }
    const float inv_n = 1.f / (float)n_rows;
    const int owner = row >= 0 ? row : 0;                     // (no camera this step: row 0's thread only zeroes the buffer)
    for (int r0 = 0; r0 < n_rows; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r < n_rows) {
#pragma unroll
            for (int i = 0; i < 6; ++i) t[i] = pose[6 * (size_t)r + i];
        }
        if (r == owner) {
            float G[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { G[i] = v_viewmats[i]; v_viewmats[i] = 0.f; }
            if (row >= 0 && !skipped) {
                float in[12], opt[12], v[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) in[i] = c2w_in[i];
                pose_compose(t, in, opt);
                viewmat_bwd(opt, G, v);
                pose_compose_bwd(t, in, v, g);
            }
        }
        if (r >= n_rows || skipped) continue;
        const float nd = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        const float nw = sqrtf(t[3] * t[3] + t[4] * t[4] + t[5] * t[5]);
        // d |x| / dx = x / |x|, and 0 at x = 0 (torch's norm backward)
        const float kd = nd > 0.f ? trans_pen * inv_n / nd : 0.f, kw = nw > 0.f ? rot_pen * inv_n / nw : 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const size_t e = 6 * (size_t)r + i;
            const float gg = g[i] + (i < 3 ? kd : kw) * t[i];
            if (raw_grad != nullptr) raw_grad[e] = gg;
            float mm = exp_avg[e], vv = exp_avg_sq[e];
            mm = co.beta1 * mm + co.omb1 * gg;
            vv = co.beta2 * vv + co.omb2 * gg * gg;
            const float denom = sqrtf(vv) * co.inv_bc2_sqrt + co.eps;
            pose[e] = t[i] - co.lr * co.inv_bc1 * mm / denom;
            exp_avg[e] = mm;
            exp_avg_sq[e] = vv;
        }
    }
}

}  // namespace qed

using namespace qed;

static bool pose_rows_ok(int32_t C, int32_t n_rows, const int32_t* rows, int32_t row0) {
    return rows != nullptr || (row0 >= 0 && (long long)row0 + C <= n_rows);
}

extern "C" int qed_pose_apply(int32_t C, int32_t n_rows, const float* pose_adjustment, const int32_t* rows, int32_t row0,
                              const float* c2w_in, float* c2w_out, float trans_l2_penalty, float rot_l2_penalty,
                              float* reg_out, void* stream) {
    QED_REQUIRE(C >= 1 && n_rows >= 1 && n_rows < (1 << 24), "C >= 1 and 1 <= n_rows < 2^24 required");
    QED_REQUIRE(pose_adjustment && c2w_in && c2w_out, "null buffer");
    QED_REQUIRE(pose_rows_ok(C, n_rows, rows, row0), "rows row0 .. row0 + C must lie inside pose_adjustment");
    hipLaunchKernelGGL(pose_apply_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C, n_rows,
                       pose_adjustment, rows, row0, c2w_in, c2w_out, trans_l2_penalty, rot_l2_penalty, reg_out);
    return check_launch("qed_pose_apply");
}

extern "C" int qed_pose_apply_bwd(int32_t C, int32_t n_rows, const float* pose_adjustment, const int32_t* rows,
                                  int32_t row0, const float* c2w_in, const float* v_c2w, float* v_rows, void* stream) {
    QED_REQUIRE(C >= 1 && n_rows >= 1 && n_rows < (1 << 24), "C >= 1 and 1 <= n_rows < 2^24 required");
    QED_REQUIRE(pose_adjustment && c2w_in && v_c2w && v_rows, "null buffer");
    QED_REQUIRE(pose_rows_ok(C, n_rows, rows, row0), "rows row0 .. row0 + C must lie inside pose_adjustment");
    hipLaunchKernelGGL(pose_apply_bwd_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C,
                       n_rows, pose_adjustment, rows, row0, c2w_in, v_c2w, v_rows);
    return check_launch("qed_pose_apply_bwd");
}

extern "C" int qed_pose_step(int32_t n_rows, int32_t row, float* pose_adjustment, float* exp_avg, float* exp_avg_sq,
                             const float* c2w_in, float* v_viewmats, float trans_l2_penalty, float rot_l2_penalty,
                             float lr, double beta1, double beta2, float eps, int32_t step, float* raw_grad,
                             float* reg_out, const int32_t* skip_flag, void* stream) {
    QED_REQUIRE(n_rows >= 1 && n_rows < (1 << 24), "1 <= n_rows < 2^24 required");
    QED_REQUIRE(row >= -1 && row < n_rows, "row must be -1 (no camera this step) or a row of pose_adjustment");
    QED_REQUIRE(pose_adjustment && exp_avg && exp_avg_sq && v_viewmats, "null buffer");
    QED_REQUIRE(row < 0 || c2w_in, "c2w_in is required with a row");
    QED_REQUIRE(step >= 1, "step is 1-based");
    PoseAdam co{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps,
                (float)(1.0 / (1.0 - pow(beta1, (double)step))), (float)(1.0 / sqrt(1.0 - pow(beta2, (double)step))), lr};
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_rows, row, pose_adjustment, exp_avg,
                       exp_avg_sq, c2w_in, v_viewmats, trans_l2_penalty, rot_l2_penalty, co, raw_grad, reg_out, skip_flag);
    return check_launch("qed_pose_step");
}
