// Normal maps at evaluation / rendering time: a Gaussian's normal, the normal image and the normals of a depth map, and the
// angular error between two normal images.  Three small kernels AROUND one more launch of the forward compositing kernel
// (composite.hip, unchanged): a Gaussian's normal rides through it in the colour slots of a second set of records, so the
// accumulated normal A(p) = Sum_i alpha_i T_i n_i has the colour image's own weights, lists and tiles -- no second
// projection, no second binning.
//
//   qed_gaussian_normals   one (camera, Gaussian) slot per thread.  The normal is the axis of the smallest scale (lowest
//                          index on a tie; compared on the values as stored: exp is monotone, so log-scales need no exp),
//                          column k of R(q / |q|), turned to face the camera (negated where dot(n, mean - o) > 0,
//                          o = -R_v^T t the camera origin), in the world frame or the OpenCV camera frame of `viewmats`
//                          (x right, y down, z forward: a facing surface has n_z < 0).  A zero quaternion gives 0.
//                          The 48-byte record is read and written as three 16-byte accesses per thread; slots 6, 7, 8
//                          (r, g, b) receive the normal, everything else is copied bit for bit.  136 B per slot (148 with
//                          normals_out).  A workgroup moves its 256 records through LDS as 768 consecutive 16-byte words:
//                          13.6 us per launch at 500 k Gaussians against 39.0 us with every thread moving its own
//                          record's three words (a kernel trace of 20 launches each, profiles/normals.txt).
//   qed_normal_maps        one pixel per thread: normal = A / |A|, the normal of the surface depth z = D / alpha by central
//   qed_depth_normals      differences of the back-projected points, the valid bits, optionally the 8-bit colouring.
//                          The stencil is evaluated in DOUBLE: P(x+1) - P(x-1) cancels all but ~1 / fx of its operands,
//                          and float32 would leave the normal of a 1080p depth map with ~1e-4 of noise; in double the
//                          result is the float64 definition's to ~1e-7 for every intrinsics.  (A few dozen f64
//                          operations per pixel: the pass stays bound by its ~60 B per pixel.)
//   qed_angular_error      atan2(|a x b|, a . b) per pixel (well conditioned at 0 and pi, where acos of a float32 dot
//                          product is not); sum, count and the counts under up to three thresholds are carried in double
//                          per thread and folded by qed_reduce.h's two-launch pattern in a fixed order: no float atomics,
//                          two runs give the same bits.
#include "qed_common.h"

namespace qed {

// ---- per-Gaussian normals ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
gaussian_normals_kernel(int N, long long total, const float* __restrict__ means, const float* __restrict__ quats,
                        const float* __restrict__ scales, const float* __restrict__ viewmats,
                        const float4* __restrict__ splats, int camera_frame, float* __restrict__ normals_out,
                        float4* __restrict__ splats_out) {
    // The workgroup's 256 records are 768 consecutive 16-byte words: thread t moves words t, t + 256 and t + 512 of them
    // (three 16-byte accesses per thread each way, consecutive lanes on consecutive addresses) through LDS, where the owner
    // of a record patches its three colour slots.  Read as r0, r1, r2 of the thread's own record the same accesses are 48
    // bytes apart from lane to lane, and a wave's request covers a third of every line it touches.
    __shared__ float4 s_rec[768];
    const long long first = (long long)blockIdx.x * 256;
    const long long slot = first + threadIdx.x;
    const bool live = slot < total;                          // (no early return: the barriers below need every thread)
    if (splats_out != nullptr) {                              // the record's loads first: they are the longest wait
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long g = 3 * first + j * 256 + threadIdx.x;
            if (g < 3 * total) s_rec[j * 256 + threadIdx.x] = splats[g];
        }
    }
    const long long ls = live ? slot : first;                 // (first < total: the grid has no empty workgroup)
    const int c = (int)(ls / N), n = (int)(ls - (long long)c * N);
    const float s0 = scales[3 * n], s1 = scales[3 * n + 1], s2 = scales[3 * n + 2];
    const float w = quats[4 * n], x = quats[4 * n + 1], y = quats[4 * n + 2], z = quats[4 * n + 3];
    const float m[3] = {means[3 * n], means[3 * n + 1], means[3 * n + 2]};
    const float* V = viewmats + 16 * (size_t)c;
    const float R[9] = {V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
    const float t[3] = {V[3], V[7], V[11]};

    int k = 0;                                                // strict <: the lowest index wins a tie
    float smin = s0;
    if (s1 < smin) { k = 1; smin = s1; }
    if (s2 < smin) k = 2;

    const float n2 = w * w + x * x + y * y + z * z;
    const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;      // (a zero quaternion: every component 0, and `unit` below)
    const float unit = n2 > 0.f ? 1.f : 0.f;
    const float qw = w * inv, qx = x * inv, qy = y * inv, qz = z * inv;
    float nw[3];                                              // column k of quat_to_rotmat (project.hip)
    if (k == 0) {
        nw[0] = unit - 2.f * (qy * qy + qz * qz); nw[1] = 2.f * (qx * qy + qw * qz); nw[2] = 2.f * (qx * qz - qw * qy);
    } else if (k == 1) {
        nw[0] = 2.f * (qx * qy - qw * qz); nw[1] = unit - 2.f * (qx * qx + qz * qz); nw[2] = 2.f * (qy * qz + qw * qx);
    } else {
        nw[0] = 2.f * (qx * qz + qw * qy); nw[1] = 2.f * (qy * qz - qw * qx); nw[2] = unit - 2.f * (qx * qx + qy * qy);
    }
    // towards the camera: o = -R^T t
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float o = -(R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]);
        d += nw[j] * (m[j] - o);
    }
    if (d > 0.f) { nw[0] = -nw[0]; nw[1] = -nw[1]; nw[2] = -nw[2]; }
    float out[3] = {nw[0], nw[1], nw[2]};
    if (camera_frame) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * nw[0] + R[3 * i + 1] * nw[1] + R[3 * i + 2] * nw[2];
    }
    if (live && normals_out != nullptr) {
        normals_out[3 * slot] = out[0]; normals_out[3 * slot + 1] = out[1]; normals_out[3 * slot + 2] = out[2];
    }
    if (splats_out != nullptr) {
        __syncthreads();
        if (live) {
            float* r = reinterpret_cast<float*>(&s_rec[3 * threadIdx.x]);
            r[6] = out[0]; r[7] = out[1]; r[8] = out[2];      // slots 6, 7, 8
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long g = 3 * first + j * 256 + threadIdx.x;
            if (g < 3 * total) splats_out[g] = s_rec[j * 256 + threadIdx.x];
        }
    }
}

// ---- the image pass ------------------------------------------------------------------------------------------------------
// surface depth of a pixel, NaN where it has none: z = D / alpha where alpha >= min_alpha (alpha == NULL: z = D); finite, > 0
__device__ __forceinline__ double surface_depth(const float* __restrict__ depth, int depth_stride,
                                                const float* __restrict__ alpha, float min_alpha, size_t p) {
    double z = (double)depth[p * (size_t)depth_stride];
    if (alpha != nullptr) {
        const float a = alpha[p];
        if (!(a >= min_alpha)) return __builtin_nan("");
        z /= (double)a;
    }
    return (isfinite(z) && z > 0.0) ? z : __builtin_nan("");
}

__device__ __forceinline__ unsigned char normal_byte(float v) {
    return (unsigned char)fminf(fmaxf(rintf(255.f * (0.5f + 0.5f * v)), 0.f), 255.f);
}

__global__ void __launch_bounds__(256)
normal_maps_kernel(int H, int W, const float* __restrict__ accum, const float* __restrict__ alpha,
                   const float* __restrict__ depth, int depth_stride, double fx, double fy, double cx, double cy,
                   float min_alpha, float* __restrict__ normal, float* __restrict__ depth_normal,
                   unsigned char* __restrict__ valid, unsigned char* __restrict__ rgb8, int rgb8_of_depth) {
    const size_t n_pix = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const int py = (int)(p / W), px = (int)(p - (size_t)py * W);
    unsigned bits = 0;

    float nr[3] = {0.f, 0.f, 0.f};
    if (accum != nullptr) {
        const float a = alpha != nullptr ? alpha[p] : 1.f;
        const float A[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
        const double len = sqrt((double)A[0] * A[0] + (double)A[1] * A[1] + (double)A[2] * A[2]);
        if (a >= min_alpha && len > 1e-8) {
            const float il = (float)(1.0 / len);
            nr[0] = A[0] * il; nr[1] = A[1] * il; nr[2] = A[2] * il;
            bits |= QED_NV_NORMAL;
        }
        if (normal != nullptr) { normal[3 * p] = nr[0]; normal[3 * p + 1] = nr[1]; normal[3 * p + 2] = nr[2]; }
    }

    float nd[3] = {0.f, 0.f, 0.f};
    if (px > 0 && py > 0 && px < W - 1 && py < H - 1) {       // (never true under 3 x 3: every pixel is a border pixel)
        const double zc = surface_depth(depth, depth_stride, alpha, min_alpha, p);
        const double zl = surface_depth(depth, depth_stride, alpha, min_alpha, p - 1);
        const double zr = surface_depth(depth, depth_stride, alpha, min_alpha, p + 1);
        const double zu = surface_depth(depth, depth_stride, alpha, min_alpha, p - W);
        const double zd = surface_depth(depth, depth_stride, alpha, min_alpha, p + W);
        if (!(isnan(zc) || isnan(zl) || isnan(zr) || isnan(zu) || isnan(zd))) {
            const double ul = ((double)(px - 1) + 0.5 - cx) / fx, ur = ((double)(px + 1) + 0.5 - cx) / fx;
            const double uc = ((double)px + 0.5 - cx) / fx;
            const double vu = ((double)(py - 1) + 0.5 - cy) / fy, vd = ((double)(py + 1) + 0.5 - cy) / fy;
            const double vc = ((double)py + 0.5 - cy) / fy;
            const double dx[3] = {ur * zr - ul * zl, vc * zr - vc * zl, zr - zl};
            const double dy[3] = {uc * zd - uc * zu, vd * zd - vu * zu, zd - zu};
            const double cr[3] = {dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2],
                                  dy[0] * dx[1] - dy[1] * dx[0]};
            const double len = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
            if (len > 1e-20) {
                nd[0] = (float)(cr[0] / len); nd[1] = (float)(cr[1] / len); nd[2] = (float)(cr[2] / len);
                bits |= QED_NV_DEPTH_NORMAL;
            }
        }
    }
    if (depth_normal != nullptr) {
        depth_normal[3 * p] = nd[0]; depth_normal[3 * p + 1] = nd[1]; depth_normal[3 * p + 2] = nd[2];
    }
    valid[p] = (unsigned char)bits;
    if (rgb8 != nullptr) {
        const float* v = rgb8_of_depth ? nd : nr;
        const bool ok = (bits & (rgb8_of_depth ? QED_NV_DEPTH_NORMAL : QED_NV_NORMAL)) != 0;
        rgb8[3 * p] = ok ? normal_byte(v[0]) : 0;             // x right -> red, y UP -> green, towards the camera -> blue
        rgb8[3 * p + 1] = ok ? normal_byte(-v[1]) : 0;
        rgb8[3 * p + 2] = ok ? normal_byte(-v[2]) : 0;
    }
}

// ---- angular error -------------------------------------------------------------------------------------------------------
constexpr int kAngCols = 5;                                   // sum of angles | count | counts under thresholds 0, 1, 2
constexpr int kAngMaxGrid = QED_ANGULAR_WS_DOUBLES / kAngCols;

__global__ void __launch_bounds__(256)
angular_error_kernel(int n_pix, const float* __restrict__ a, const float* __restrict__ b,
                     const unsigned char* __restrict__ valid_a, unsigned bits_a, const unsigned char* __restrict__ valid_b,
                     unsigned bits_b, const unsigned char* __restrict__ mask, int n_thr, float t0, float t1, float t2,
                     float* __restrict__ angle, double* __restrict__ partials) {
    double acc[kAngCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // kU pixels per trip, every load of the trip issued before the first use (clamped index, the pixel switched off by
    // `in`), the shape metrics.hip's pass has: with at most 1024 workgroups a thread walks ~8 pixels at 1080p, one
    // dependent memory round trip each otherwise.  16.4 us per launch at 1080p (62 MB needed: 3.8 TB/s; profiles/normals.txt).
    constexpr int kU = 4;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < (size_t)n_pix; i0 += kU * stride) {
        float av[kU][3], bv[kU][3];
        bool ok[kU], in[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const size_t iu = i0 + u * stride;
            in[u] = iu < (size_t)n_pix;
            const size_t i = in[u] ? iu : i0;
            ok[u] = in[u] && (valid_a[i] & bits_a) != 0 && (valid_b[i] & bits_b) != 0 && (mask == nullptr || mask[i] != 0);
#pragma unroll
            for (int k = 0; k < 3; ++k) { av[u][k] = a[3 * i + k]; bv[u][k] = b[3 * i + k]; }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {                        // (in index order: the sums' order is fixed)
            if (!in[u]) continue;
            float ang = __builtin_nanf("");
            if (ok[u]) {
                const float ax = av[u][0], ay = av[u][1], az = av[u][2];
                const float bx = bv[u][0], by = bv[u][1], bz = bv[u][2];
                const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
                ang = atan2f(sqrtf(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
                acc[0] += (double)ang;
                acc[1] += 1.0;
                if (n_thr > 0 && ang < t0) acc[2] += 1.0;
                if (n_thr > 1 && ang < t1) acc[3] += 1.0;
                if (n_thr > 2 && ang < t2) acc[4] += 1.0;
            }
            if (angle != nullptr) angle[i0 + u * stride] = ang;
        }
    }
    __shared__ double s_w[kAngCols][4];
    __shared__ double s[kAngCols];
    block_sum_d(acc, s_w, s);
    if (threadIdx.x < kAngCols) partials[(size_t)threadIdx.x * kAngMaxGrid + blockIdx.x] = s[threadIdx.x];
}

__global__ void __launch_bounds__(256)
angular_error_finalize_kernel(int n_blocks, const double* __restrict__ partials, double* __restrict__ out) {
    __shared__ double s_w[kAngCols][4];
    __shared__ double s[kAngCols];
    double v[kAngCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int blk = threadIdx.x; blk < n_blocks; blk += 256) {
#pragma unroll
        for (int c = 0; c < kAngCols; ++c) v[c] += partials[(size_t)c * kAngMaxGrid + blk];
    }
    block_sum_d(v, s_w, s);
    if (threadIdx.x < kAngCols) out[threadIdx.x] = s[threadIdx.x];
}

static int launch_normal_maps(const char* who, int32_t height, int32_t width, const float* accum, const float* alpha,
                              const float* depth, int32_t depth_stride, float fx, float fy, float cx, float cy,
                              float min_alpha, float* normal, float* depth_normal, uint8_t* valid, uint8_t* rgb8,
                              int rgb8_of_depth, void* stream) {
    const long long n_pix = (long long)height * width;
    const long long grid = (n_pix + 255) / 256;
    if (grid > 0x7fffffffLL) {
        set_error("%s: image too large", who);
        return QED_E_INVALID_ARG;
    }
    hipLaunchKernelGGL(normal_maps_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, height, width, accum,
                       alpha, depth, depth_stride, (double)fx, (double)fy, (double)cx, (double)cy, min_alpha, normal,
                       depth_normal, valid, rgb8, rgb8_of_depth);
    return check_launch(who);
}

}  // namespace qed

using namespace qed;

extern "C" int qed_gaussian_normals(int32_t N, int32_t C, const float* means, const float* quats, const float* scales,
                                    const float* viewmats, const float* splats, int32_t frame, uint32_t flags,
                                    float* normals_out, float* splats_out, void* stream) {
    (void)flags;                                              // QED_F_LOG_SCALES: the order of the logarithms is the scales'
    QED_REQUIRE(N >= 0 && C >= 0, "negative size");
    QED_REQUIRE(frame == QED_NORMALS_WORLD || frame == QED_NORMALS_CAMERA, "frame: QED_NORMALS_WORLD or QED_NORMALS_CAMERA");
    const long long total = (long long)N * C;
    if (total == 0) return QED_OK;
    QED_REQUIRE(means && quats && scales && viewmats, "null input");
    QED_REQUIRE(normals_out || splats_out, "no output");
    QED_REQUIRE(splats_out == nullptr || splats != nullptr, "splats_out needs splats");
    QED_REQUIRE((((uintptr_t)splats | (uintptr_t)splats_out) & 15) == 0, "records must be 16-byte aligned");
    const long long grid = (total + 255) / 256;
    QED_REQUIRE(grid <= 0x7fffffffLL, "too many slots");
    hipLaunchKernelGGL(gaussian_normals_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, N, total, means,
                       quats, scales, viewmats, (const float4*)splats, frame == QED_NORMALS_CAMERA ? 1 : 0, normals_out,
                       (float4*)splats_out);
    return check_launch("qed_gaussian_normals");
}

extern "C" int qed_normal_maps(int32_t height, int32_t width, const float* accum, const float* alpha, const float* depth,
                               int32_t depth_stride, float fx, float fy, float cx, float cy, float min_alpha, float* normal,
                               float* depth_normal, uint8_t* valid, uint8_t* rgb8, void* stream) {
    QED_REQUIRE(height >= 0 && width >= 0 && depth_stride >= 1, "bad sizes");
    if (height == 0 || width == 0) return QED_OK;
    QED_REQUIRE(depth && valid, "null pointer");
    QED_REQUIRE(accum == nullptr || alpha != nullptr, "an accumulated normal needs its alpha");
    QED_REQUIRE(normal == nullptr || accum != nullptr, "normal needs the accumulated normal");
    QED_REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    return launch_normal_maps("qed_normal_maps", height, width, accum, alpha, depth, depth_stride, fx, fy, cx, cy, min_alpha,
                              normal, depth_normal, valid, rgb8, accum == nullptr, stream);
}

extern "C" int qed_depth_normals(int32_t height, int32_t width, const float* depth, int32_t depth_stride, float fx, float fy,
                                 float cx, float cy, float* depth_normal, uint8_t* valid, uint8_t* rgb8, void* stream) {
    QED_REQUIRE(height >= 0 && width >= 0 && depth_stride >= 1, "bad sizes");
    if (height == 0 || width == 0) return QED_OK;
    QED_REQUIRE(depth && valid, "null pointer");
    QED_REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    return launch_normal_maps("qed_depth_normals", height, width, nullptr, nullptr, depth, depth_stride, fx, fy, cx, cy, 0.f,
                              nullptr, depth_normal, valid, rgb8, 1, stream);
}

extern "C" int qed_angular_error(int32_t n_pix, const float* a, const float* b, const uint8_t* valid_a, uint32_t bits_a,
                                 const uint8_t* valid_b, uint32_t bits_b, const uint8_t* mask, int32_t n_thresholds,
                                 float t0, float t1, float t2, double* workspace, float* angle, double* out, void* stream) {
    QED_REQUIRE(n_pix >= 0 && n_thresholds >= 0 && n_thresholds <= 3, "bad sizes (thresholds: 0 to 3)");
    QED_REQUIRE(workspace && out, "null pointer");
    QED_REQUIRE(n_pix == 0 || (a && b && valid_a && valid_b), "null input");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "misaligned double pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = n_pix == 0 ? 0u : stream_grid(n_pix, kAngMaxGrid);
    if (grid > 0)
        hipLaunchKernelGGL(angular_error_kernel, dim3(grid), dim3(256), 0, st, n_pix, a, b, valid_a, bits_a, valid_b, bits_b,
                           mask, n_thresholds, t0, t1, t2, angle, workspace);
    hipLaunchKernelGGL(angular_error_finalize_kernel, dim3(1), dim3(256), 0, st, (int)grid, (const double*)workspace, out);
    return check_launch("qed_angular_error");
}
