// Oriented surface samples of one rendered view: the rendered depth and a normal plane back-projected into a compact list of
// world points with normals and colours -- what a Poisson tool or PDMetrics takes.  No intermediate image is written.
//
// Contract (include/qed_splat.h states it; the ORDER of the operations is part of it).  For every stride-th pixel (x, y):
//   1. alpha >= min_alpha and, with a mask, mask != 0;
//   2. z = D / alpha finite with depth_min <= z <= depth_max;
//   3. the chosen normal n (rendered or depth normal) carries its QED_NV_* bit;
//   4. agreement filter (cos_max_normal_angle > -1) where BOTH normals are valid: dot(normal, depth_normal) >= the cosine;
//   5. P = ((x + .5 - cx) z / fx, (y + .5 - cy) z / fy, z): the renderer's pixel centres, as qed_normal_maps;
//   6. grazing filter (min_view_cos > 0): -dot(n, P / |P|) >= min_view_cos;
//   7. world point R^T (P - t), world normal R^T n of the OpenCV world-to-camera matrix [R | t].
// Everything is evaluated in double from the float32 inputs and rounded to float32 once.
//
// Three launches, like qed_backproject_depth: (1) every thread decides its pixel, a wave's decisions go to the workspace as
// one 64-bit word and the workgroup's count beside it; (2) qed_isect_scan turns the counts into offsets and reports a
// list longer than the caller's buffers; (3) the kept pixels are evaluated again (no filter: the word decides) and written in
// row-major pixel order.  No atomic counter: two calls give the same bits.
//
// Memory shape of (3): at stride 1 a workgroup's 256 pixels are 768 consecutive floats of a [H,W,3] plane, fetched as 192
// 16-byte loads into LDS (the colour and the chosen normal); a thread reading its own 12-byte row would spread every wave
// request over three times the lines it uses.  The three outputs are 12-byte rows at a rank only known after the count, so
// they are staged in LDS by rank and leave as consecutive dwords from consecutive lanes.
#include "qed_common.h"

#include <math.h>

extern "C" int qed_isect_scan(const int32_t* block_sums, int32_t n_blocks, int32_t* block_offsets, int32_t* n_isect,
                              int64_t capacity, int32_t* status, void* stream);

namespace qed {

constexpr int kSurfThreads = 256;
constexpr int kSurfRow = 3 * kSurfThreads;          // floats of one workgroup's rows in a [.,3] plane

struct SurfaceArgs {
    int W, stride, gw;                               // gw = strided pixels per row
    long long g;                                     // strided pixels in all
    int depth_stride, use_depth_normal;
    double fx, fy, cx, cy;
    float min_alpha, depth_min, depth_max, cos_max_normal_angle, min_view_cos;
};

struct SurfacePlanes {
    const float *rgb, *depth, *alpha, *normal, *depth_normal, *viewmat;
    const unsigned char *valid, *mask;
};

// strided pixel i -> (x, y) and the pixel's index in the planes
__device__ __forceinline__ size_t surf_pixel(const SurfaceArgs& a, long long i, int& x, int& y) {
    const int gy = (int)(i / a.gw), gx = (int)(i - (long long)gy * a.gw);
    x = gx * a.stride; y = gy * a.stride;
    return (size_t)y * a.W + x;
}

// steps 1 and 2: the surface depth of pixel p, NaN where the pixel has none
__device__ __forceinline__ double surf_depth(const SurfaceArgs& a, const SurfacePlanes& s, size_t p) {
    const float al = s.alpha[p];
    if (!(al >= a.min_alpha)) return __builtin_nan("");
    if (s.mask != nullptr && s.mask[p] == 0) return __builtin_nan("");
    const double z = (double)s.depth[p * (size_t)a.depth_stride] / (double)al;
    return (isfinite(z) && z >= (double)a.depth_min && z <= (double)a.depth_max) ? z : __builtin_nan("");
}

// step 5
__device__ __forceinline__ void surf_point(const SurfaceArgs& a, int x, int y, double z, double P[3]) {
    P[0] = ((double)x + 0.5 - a.cx) * z / a.fx;
    P[1] = ((double)y + 0.5 - a.cy) * z / a.fy;
    P[2] = z;
}

// ---- (1) decide ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSurfThreads)
surface_count_kernel(SurfaceArgs a, SurfacePlanes s, int* __restrict__ block_counts, int* __restrict__ keep_words,
                     int* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x < QED_STATUS_WORDS) status[threadIdx.x] = 0;
    const long long i = (long long)blockIdx.x * kSurfThreads + threadIdx.x;
    bool keep = false;
    if (i < a.g) {
        int x, y;
        const size_t p = surf_pixel(a, i, x, y);
        const double z = surf_depth(a, s, p);
        const unsigned bits = s.valid[p];
        const unsigned want = a.use_depth_normal ? QED_NV_DEPTH_NORMAL : QED_NV_NORMAL;
        keep = !isnan(z) && (bits & want) != 0;
        const bool agree = a.cos_max_normal_angle > -1.f &&
                           (bits & (QED_NV_NORMAL | QED_NV_DEPTH_NORMAL)) == (QED_NV_NORMAL | QED_NV_DEPTH_NORMAL);
        const bool graze = a.min_view_cos > 0.f;
        if (keep && (agree || graze)) {
            double nr[3], nd[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { nr[k] = (double)s.normal[3 * p + k]; nd[k] = (double)s.depth_normal[3 * p + k]; }
            if (agree) keep = nr[0] * nd[0] + nr[1] * nd[1] + nr[2] * nd[2] >= (double)a.cos_max_normal_angle;
            if (keep && graze) {
                const double* n = a.use_depth_normal ? nd : nr;
                double P[3];
                surf_point(a, x, y, z, P);
                const double len = sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
                keep = -(n[0] * (P[0] / len) + n[1] * (P[1] / len) + n[2] * (P[2] / len)) >= (double)a.min_view_cos;
            }
        }
    }
    __shared__ int s_cnt[kSurfThreads / 64];
    const unsigned long long m = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[wave] = __popcll(m);
        const size_t w = ((size_t)blockIdx.x * (kSurfThreads / 64) + wave) * 2;
        keep_words[w] = (int)(unsigned)(m & 0xffffffffull);
        keep_words[w + 1] = (int)(unsigned)(m >> 32);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---- (3) write ----------------------------------------------------------------------------------------------------------
// DENSE: stride 1 and 16-byte aligned planes -- strided pixel i is pixel i, and the workgroup's rows of a [.,3] plane are the
// floats [768 b, 768 b + 768) of it
template <bool DENSE>
__global__ void __launch_bounds__(kSurfThreads)
surface_write_kernel(SurfaceArgs a, SurfacePlanes s, const int* __restrict__ block_counts,
                     const int* __restrict__ block_offsets, const int* __restrict__ keep_words,
                     const int* __restrict__ n_out, float* __restrict__ points, float* __restrict__ normals,
                     float* __restrict__ colors) {
    if (n_out[0] == 0) return;                          // nothing kept, or the buffers were too small
    const int count = block_counts[blockIdx.x];
    if (count == 0) return;                             // (uniform: no barrier is skipped by part of a workgroup)
    __shared__ float s_in[2][kSurfRow];                 // DENSE: the colour rows, the chosen normal's rows
    __shared__ float s_out[3][kSurfRow];                // points, normals, colours by rank
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* normal_plane = a.use_depth_normal ? s.depth_normal : s.normal;
    if (DENSE) {
        const long long f0 = (long long)blockIdx.x * kSurfRow, f_end = 3 * a.g;          // floats of the planes
        const float* src[2] = {s.rgb, normal_plane};
        if (tid < kSurfRow / 4) {
            const long long f = f0 + 4 * tid;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (f + 4 <= f_end) {
                    *reinterpret_cast<float4*>(&s_in[q][4 * tid]) = *reinterpret_cast<const float4*>(src[q] + f);
                } else {
                    for (int k = 0; k < 4; ++k)
                        if (f + k < f_end) s_in[q][4 * tid + k] = src[q][f + k];
                }
            }
        }
    }
    // my rank among the workgroup's kept pixels, from the words of (1)
    int rank = 0;
    bool keep = false;
#pragma unroll
    for (int w = 0; w < kSurfThreads / 64; ++w) {
        const size_t at = ((size_t)blockIdx.x * (kSurfThreads / 64) + w) * 2;
        const unsigned long long m = (unsigned long long)(unsigned)keep_words[at] |
                                     ((unsigned long long)(unsigned)keep_words[at + 1] << 32);
        if (w < wave) rank += __popcll(m);
        if (w == wave) { rank += __popcll(m & ((1ull << lane) - 1ull)); keep = (m >> lane) & 1ull; }
    }
    if (DENSE) __syncthreads();
    if (keep) {
        const long long i = (long long)blockIdx.x * kSurfThreads + tid;
        int x, y;
        const size_t p = surf_pixel(a, i, x, y);
        const double z = (double)s.depth[p * (size_t)a.depth_stride] / (double)s.alpha[p];
        double P[3], n[3];
        float c[3];
        surf_point(a, x, y, z, P);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = DENSE ? s_in[0][3 * tid + k] : s.rgb[3 * p + k];
            n[k] = (double)(DENSE ? s_in[1][3 * tid + k] : normal_plane[3 * p + k]);
        }
        const float* V = s.viewmat;
        const double d[3] = {P[0] - (double)V[3], P[1] - (double)V[7], P[2] - (double)V[11]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {                  // column j of R: R^T (P - t), R^T n
            const double r0 = (double)V[j], r1 = (double)V[4 + j], r2 = (double)V[8 + j];
            s_out[0][3 * rank + j] = (float)(r0 * d[0] + r1 * d[1] + r2 * d[2]);
            s_out[1][3 * rank + j] = (float)(r0 * n[0] + r1 * n[1] + r2 * n[2]);
            s_out[2][3 * rank + j] = c[j];
        }
    }
    __syncthreads();
    const size_t base = 3 * (size_t)block_offsets[blockIdx.x];           // (offset + count <= n_out <= capacity)
    for (int j = tid; j < 3 * count; j += kSurfThreads) {
        points[base + j] = s_out[0][j];
        normals[base + j] = s_out[1][j];
        colors[base + j] = s_out[2][j];
    }
}

static long long surface_blocks(int height, int width, int stride) {
    const long long g = (long long)((width + stride - 1) / stride) * ((height + stride - 1) / stride);
    return (g + kSurfThreads - 1) / kSurfThreads;
}

}  // namespace qed

using namespace qed;

// per workgroup: its count, its offset, and the four 64-bit decision words of its waves
extern "C" int64_t qed_surface_workspace_ints(int32_t height, int32_t width, int32_t stride) {
    if (height < 0 || width < 0 || stride < 1 || (long long)height * width > 0x7fffffffLL) return QED_E_INVALID_ARG;
    return (2 + 2 * (kSurfThreads / 64)) * surface_blocks(height, width, stride) + 8;
}

extern "C" int qed_surface_samples(int32_t height, int32_t width, const float* rgb, const float* depth, int32_t depth_stride,
                                   const float* alpha, const float* normal, const float* depth_normal, const uint8_t* valid,
                                   const uint8_t* mask, float fx, float fy, float cx, float cy, const float* viewmat,
                                   int32_t stride, float min_alpha, float depth_min, float depth_max, int32_t normal_source,
                                   float cos_max_normal_angle, float min_view_cos, int64_t capacity, float* points,
                                   float* normals, float* colors, int32_t* n_out, int32_t* workspace, int64_t workspace_ints,
                                   int32_t* status, void* stream) {
    QED_REQUIRE(height >= 0 && width >= 0 && (long long)height * width <= 0x7fffffffLL, "bad image size");
    QED_REQUIRE(stride >= 1, "stride must be at least 1");
    QED_REQUIRE(depth_stride >= 1, "depth_stride must be at least 1");
    QED_REQUIRE(capacity >= 0 && capacity <= 0x7fffffffLL, "capacity out of range");
    QED_REQUIRE(isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy), "intrinsics must be finite");
    QED_REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    QED_REQUIRE(depth_min <= depth_max, "depth_min must not exceed depth_max");
    QED_REQUIRE(normal_source == QED_SURFACE_NORMAL_RENDERED || normal_source == QED_SURFACE_NORMAL_DEPTH,
                "normal_source: QED_SURFACE_NORMAL_RENDERED or QED_SURFACE_NORMAL_DEPTH");
    if (height == 0 || width == 0) return QED_OK;
    QED_REQUIRE(rgb && depth && alpha && normal && depth_normal && valid && viewmat && n_out && workspace && status,
                "null buffers");
    QED_REQUIRE(capacity == 0 || (points && normals && colors), "null buffers");
    const long long nb = surface_blocks(height, width, stride);
    const long long need = (2 + 2 * (kSurfThreads / 64)) * nb + 8;
    if (workspace_ints < need) {
        set_error("qed_surface_samples: workspace too small (%lld < %lld ints)", (long long)workspace_ints, need);
        return QED_E_WORKSPACE;
    }
    SurfaceArgs a;
    a.W = width; a.stride = stride; a.gw = (width + stride - 1) / stride;
    a.g = (long long)a.gw * ((height + stride - 1) / stride);
    a.depth_stride = depth_stride;
    a.use_depth_normal = normal_source == QED_SURFACE_NORMAL_DEPTH ? 1 : 0;
    a.fx = (double)fx; a.fy = (double)fy; a.cx = (double)cx; a.cy = (double)cy;
    a.min_alpha = min_alpha; a.depth_min = depth_min; a.depth_max = depth_max;
    a.cos_max_normal_angle = cos_max_normal_angle; a.min_view_cos = min_view_cos;
    const SurfacePlanes s = {rgb, depth, alpha, normal, depth_normal, viewmat, valid, mask};
    int* block_counts = workspace;
    int* block_offsets = workspace + nb;
    int* keep_words = workspace + 2 * nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(surface_count_kernel, dim3((unsigned)nb), dim3(kSurfThreads), 0, st, a, s, block_counts, keep_words,
                       status);
    const int rc = qed_isect_scan(block_counts, (int)nb, block_offsets, n_out, capacity, status, stream);
    if (rc != QED_OK) return rc;
    const float* chosen = a.use_depth_normal ? depth_normal : normal;
    const bool dense = stride == 1 && (((uintptr_t)rgb | (uintptr_t)chosen) & 15) == 0;
    if (dense)
        hipLaunchKernelGGL(surface_write_kernel<true>, dim3((unsigned)nb), dim3(kSurfThreads), 0, st, a, s,
                           (const int*)block_counts, (const int*)block_offsets, (const int*)keep_words, (const int*)n_out,
                           points, normals, colors);
    else
        hipLaunchKernelGGL(surface_write_kernel<false>, dim3((unsigned)nb), dim3(kSurfThreads), 0, st, a, s,
                           (const int*)block_counts, (const int*)block_offsets, (const int*)keep_words, (const int*)n_out,
                           points, normals, colors);
    return check_launch("qed_surface_samples");
}
