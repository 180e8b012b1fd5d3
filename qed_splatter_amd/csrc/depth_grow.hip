// Growing Gaussians from sensor depth: where one view's render misses the surface its depth image measures, new Gaussians
// are seeded at the measured points.  Two entry points; include/qed_splat.h states both contracts.
//
// qed_depth_grow_candidates: for every stride-th pixel (x, y), in row-major order, with d = gt_depth:
//   1. measurement: d finite, d > 0, depth_min <= d <= depth_max, and (no mask or mask != 0);
//   2. HOLE: alpha < hole_alpha; else (alpha >= hole_alpha) BEHIND: z = D / alpha finite and
//      z > d + max(depth_tol, depth_tol_rel * d).  The hole test comes first: alpha == 0 never divides.
// All comparisons in double on the float32 inputs.  K candidates; with cap = capacity, f(j) = j when K <= cap and
// floor(j cap / K) otherwise: candidate j (pixel order) is kept iff f(j + 1) > f(j) and goes to row f(j) -- exactly
// min(K, cap) rows, spread evenly in pixel order.  f is monotone, so the rows of a workgroup whose candidates are
// [off, off + count) are the contiguous range [f(off), f(off + count)): they are staged in LDS by row and leave as
// consecutive dwords from consecutive lanes.
//
// Three launches, like qed_surface_samples: (1) every thread decides its pixel; a wave's decisions go to the workspace as one
// 64-bit word, the workgroup's candidate and hole counts beside it; (2) qed_isect_scan turns the counts into offsets and K;
// (3) the candidates are evaluated again (no test: the word decides), thinned and written.  Workgroup 0 of (3) also folds
// the per-workgroup hole counts (a few thousand L2-resident ints, summed in index order) and writes n_out and the status
// words.  No atomic counter anywhere: two calls give the same bits.
//
// Only the candidates read their colour (12 bytes at a data-dependent pixel), and candidates are the exception in a view
// that is mostly explained, so the colour plane is not staged as qed_surface_samples stages it.
//
// qed_grow_append: one streaming launch over the elements of the NEW flat buffers.  An element of an old row is copied
// from the same offset inside its group (three loads, three stores); an element of a new row is formed from the candidate
// rows.  Group begins are multiples of N and N + k floats, so neither side is 16-byte aligned in general: one dword per
// lane, consecutive lanes on consecutive addresses, four independent elements per thread in flight.
#include "qed_common.h"

#include <math.h>

extern "C" int qed_isect_scan(const int32_t* block_sums, int32_t n_blocks, int32_t* block_offsets, int32_t* n_isect,
                              int64_t capacity, int32_t* status, void* stream);

namespace qed {

constexpr int kGrowThreads = 256;
constexpr int kGrowWaves = kGrowThreads / 64;
constexpr int kGrowTail = 8;                         // workspace words behind the per-workgroup arrays: [0] = K, [4..8) scan status

struct GrowArgs {
    int W, stride, gw;                               // gw = strided pixels per row
    long long g;                                     // strided pixels in all
    int depth_stride;
    double fx, fy, cx, cy;
    double hole_alpha, depth_tol, depth_tol_rel, depth_min, depth_max, scale_factor;   // (float32 values, compared in double)
    long long capacity;
};

struct GrowPlanes {
    const float *gt_rgb, *gt_depth, *depth, *alpha, *viewmat;
    const unsigned char* mask;
};

__device__ __forceinline__ size_t grow_pixel(const GrowArgs& a, long long i, int& x, int& y) {
    const int gy = (int)(i / a.gw), gx = (int)(i - (long long)gy * a.gw);
    x = gx * a.stride; y = gy * a.stride;
    return (size_t)y * a.W + x;
}

// 0: no candidate, 1: hole, 2: behind
__device__ __forceinline__ int grow_decide(const GrowArgs& a, const GrowPlanes& s, size_t p) {
    const double d = (double)s.gt_depth[p];
    if (!(isfinite(d) && d > 0.0 && d >= a.depth_min && d <= a.depth_max)) return 0;
    if (s.mask != nullptr && s.mask[p] == 0) return 0;
    const double al = (double)s.alpha[p];
    if (al < a.hole_alpha) return 1;
    if (!(al >= a.hole_alpha)) return 0;             // (NaN alpha)
    const double z = (double)s.depth[p * (size_t)a.depth_stride] / al;
    if (!isfinite(z)) return 0;
    const double rel = a.depth_tol_rel * d;          // (a product of its own: never contracted into the sum below)
    return z > d + fmax(a.depth_tol, rel) ? 2 : 0;
}

// f of the header comment
__device__ __forceinline__ long long grow_row(long long j, long long K, long long cap) {
    return K <= cap ? j : j * cap / K;               // (j <= K < 2^31 and cap < 2^31: the product fits 64 bits)
}

// ---- (1) decide ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGrowThreads)
grow_count_kernel(GrowArgs a, GrowPlanes s, int* __restrict__ block_counts, int* __restrict__ block_holes,
                  int* __restrict__ keep_words) {
    const long long i = (long long)blockIdx.x * kGrowThreads + threadIdx.x;
    int kind = 0;
    if (i < a.g) {
        int x, y;
        kind = grow_decide(a, s, grow_pixel(a, i, x, y));
    }
    __shared__ int s_cnt[2][kGrowWaves];
    const unsigned long long m = __ballot(kind != 0), mh = __ballot(kind == 1);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[0][wave] = __popcll(m);
        s_cnt[1][wave] = __popcll(mh);
        const size_t w = ((size_t)blockIdx.x * kGrowWaves + wave) * 2;
        keep_words[w] = (int)(unsigned)(m & 0xffffffffull);
        keep_words[w + 1] = (int)(unsigned)(m >> 32);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        block_holes[blockIdx.x] = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    }
}

// ---- (3) thin and write -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGrowThreads)
grow_write_kernel(GrowArgs a, GrowPlanes s, int n_blocks, const int* __restrict__ block_counts,
                  const int* __restrict__ block_offsets, const int* __restrict__ block_holes,
                  const int* __restrict__ keep_words, const int* __restrict__ k_total, float* __restrict__ points,
                  float* __restrict__ log_scale, float* __restrict__ colors, int* __restrict__ n_out,
                  int* __restrict__ status) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long K = k_total[0], cap = a.capacity;
    __shared__ int s_holes[kGrowWaves];
    if (blockIdx.x == 0) {                              // the call's counts: every workgroup's holes, in index order
        int h = 0;
        for (int b = tid; b < n_blocks; b += kGrowThreads) h += block_holes[b];
        h = wave_sum_i(h);
        if (lane == 0) s_holes[wave] = h;
        __syncthreads();
        if (tid == 0) {
            const int holes = s_holes[0] + s_holes[1] + s_holes[2] + s_holes[3];
            n_out[0] = (int)(K < cap ? K : cap);
            status[0] = (int)K; status[1] = holes; status[2] = (int)K - holes;
            for (int w = 3; w < QED_STATUS_WORDS; ++w) status[w] = 0;
        }
    }
    const int count = block_counts[blockIdx.x];
    if (count == 0) return;                             // (uniform: no barrier is skipped by part of a workgroup)
    const long long off = block_offsets[blockIdx.x];
    const long long row0 = grow_row(off, K, cap);
    const int n_rows = (int)(grow_row(off + count, K, cap) - row0);       // <= count <= 256
    if (n_rows == 0) return;                            // (uniform)
    __shared__ float s_out[7][kGrowThreads];            // by row: point xyz, colour rgb, log-scale
    // my rank among the workgroup's candidates, from the words of (1)
    int rank = 0;
    bool cand = false;
#pragma unroll
    for (int w = 0; w < kGrowWaves; ++w) {
        const size_t at = ((size_t)blockIdx.x * kGrowWaves + w) * 2;
        const unsigned long long m = (unsigned long long)(unsigned)keep_words[at] |
                                     ((unsigned long long)(unsigned)keep_words[at + 1] << 32);
        if (w < wave) rank += __popcll(m);
        if (w == wave) { rank += __popcll(m & ((1ull << lane) - 1ull)); cand = (m >> lane) & 1ull; }
    }
    if (cand) {
        const long long j = off + rank;
        const long long r = grow_row(j, K, cap);
        if (grow_row(j + 1, K, cap) > r) {              // kept: the last candidate of its row
            const int q = (int)(r - row0);              // 0 <= q < n_rows
            const long long i = (long long)blockIdx.x * kGrowThreads + tid;
            int x, y;
            const size_t p = grow_pixel(a, i, x, y);
            const double d = (double)s.gt_depth[p];
            const float* V = s.viewmat;
            {
#pragma clang fp contract(off)
                const double P[3] = {((double)x + 0.5 - a.cx) * d / a.fx, ((double)y + 0.5 - a.cy) * d / a.fy, d};
                const double e[3] = {P[0] - (double)V[3], P[1] - (double)V[7], P[2] - (double)V[11]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {           // column c of R: R^T (P - t)
                    const double r0 = (double)V[c], r1 = (double)V[4 + c], r2 = (double)V[8 + c];
                    s_out[c][q] = (float)(r0 * e[0] + r1 * e[1] + r2 * e[2]);
                    s_out[3 + c][q] = s.gt_rgb[3 * p + c];
                }
                s_out[6][q] = (float)log(a.scale_factor * (double)a.stride * d / (0.5 * (a.fx + a.fy)));
            }
        }
    }
    __syncthreads();
    const size_t base = (size_t)row0;                   // (row0 + n_rows <= min(K, cap) <= capacity)
    for (int e = tid; e < 3 * n_rows; e += kGrowThreads) {
        const int q = e / 3, c = e - 3 * q;
        points[3 * base + e] = s_out[c][q];
        colors[3 * base + e] = s_out[3 + c][q];
    }
    if (tid < n_rows) log_scale[base + tid] = s_out[6][tid];
}

static long long grow_blocks(int height, int width, int stride) {
    const long long g = (long long)((width + stride - 1) / stride) * ((height + stride - 1) / stride);
    return (g + kGrowThreads - 1) / kGrowThreads;
}

// ---- append -------------------------------------------------------------------------------------------------------------
struct AppendArgs {
    EmitLayout L;                                       // begins and widths of the old (n rows) and new (n + k rows) buffers
    long long n, total;                                 // old rows; floats of a new buffer
    int sh_coeffs;
    float opacity_logit;
};

__device__ __forceinline__ float grow_new_value(const AppendArgs& a, int g, long long row, int col,
                                                const float* __restrict__ points, const float* __restrict__ log_scale,
                                                const float* __restrict__ colors) {
    switch (g) {
        case 0: return points[3 * row + col];
        case 1: return log_scale[row];
        case 2: return col == 0 ? 1.f : 0.f;
        case 3: return a.opacity_logit;
        case 4: {                                       // qed_seed_gaussians' rule, on a float colour
            const double x = (double)colors[3 * row + col];
            if (a.sh_coeffs > 1) return (float)((x - 0.5) / 0.28209479177387814);
            const double y = fmin(fmax(x, 1e-10), 1.0 - 1e-10);
            return (float)log(y / (1.0 - y));
        }
        default: return 0.f;
    }
}

__global__ void __launch_bounds__(kGrowThreads)
grow_append_kernel(AppendArgs a, const float* __restrict__ old_p, const float* __restrict__ old_m,
                   const float* __restrict__ old_v, const float* __restrict__ points, const float* __restrict__ log_scale,
                   const float* __restrict__ colors, float* __restrict__ new_p, float* __restrict__ new_m,
                   float* __restrict__ new_v) {
    constexpr int kPer = 4;
    const long long step = (long long)gridDim.x * kGrowThreads * kPer;
    for (long long e0 = (long long)blockIdx.x * kGrowThreads * kPer + threadIdx.x; e0 < a.total; e0 += step) {
        float p[kPer], m[kPer], v[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const long long e = e0 + (long long)u * kGrowThreads;
            p[u] = m[u] = v[u] = 0.f;
            if (e >= a.total) continue;
            int g = 0;
#pragma unroll
            for (int q = 1; q < 6; ++q) g += e >= a.L.new_begin[q] ? 1 : 0;
            const long long local = e - a.L.new_begin[g], n_old = a.n * a.L.width[g];
            if (local < n_old) {                        // an old row: the same offset inside the old group
                const long long src = a.L.old_begin[g] + local;
                p[u] = old_p[src]; m[u] = old_m[src]; v[u] = old_v[src];
            } else {
                const long long t = local - n_old, row = t / a.L.width[g];
                p[u] = grow_new_value(a, g, row, (int)(t - row * a.L.width[g]), points, log_scale, colors);
            }
        }
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const long long e = e0 + (long long)u * kGrowThreads;
            if (e < a.total) { new_p[e] = p[u]; new_m[e] = m[u]; new_v[e] = v[u]; }
        }
    }
}

}  // namespace qed

using namespace qed;

// per workgroup: its candidate count, its offset, its hole count and the four 64-bit decision words of its waves
extern "C" int64_t qed_depth_grow_workspace_ints(int32_t height, int32_t width, int32_t stride) {
    if (height < 0 || width < 0 || stride < 1 || (long long)height * width > 0x7fffffffLL) return QED_E_INVALID_ARG;
    return (3 + 2 * kGrowWaves) * grow_blocks(height, width, stride) + kGrowTail;
}

extern "C" int qed_depth_grow_candidates(int32_t height, int32_t width, const float* gt_rgb, const float* gt_depth,
                                         const uint8_t* mask, const float* depth, int32_t depth_stride, const float* alpha,
                                         float fx, float fy, float cx, float cy, const float* viewmat, int32_t stride,
                                         float hole_alpha, float depth_tol, float depth_tol_rel, float depth_min,
                                         float depth_max, float scale_factor, int64_t capacity, float* points,
                                         float* log_scale, float* colors, int32_t* n_out, int32_t* workspace,
                                         int64_t workspace_ints, int32_t* status, void* stream) {
    QED_REQUIRE(height >= 0 && width >= 0 && (long long)height * width <= 0x7fffffffLL, "bad image size");
    QED_REQUIRE(stride >= 1, "stride must be at least 1");
    QED_REQUIRE(depth_stride >= 1, "depth_stride must be at least 1");
    QED_REQUIRE(capacity >= 0 && capacity <= 0x7fffffffLL, "capacity out of range");
    QED_REQUIRE(isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy), "intrinsics must be finite");
    QED_REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    QED_REQUIRE(depth_min <= depth_max, "depth_min must not exceed depth_max");
    QED_REQUIRE(depth_tol >= 0.f && depth_tol_rel >= 0.f, "the depth tolerances must not be negative");
    QED_REQUIRE(hole_alpha == hole_alpha, "hole_alpha must not be NaN");
    QED_REQUIRE(scale_factor > 0.f && isfinite(scale_factor), "scale_factor must be positive and finite");
    if (height == 0 || width == 0) return QED_OK;
    QED_REQUIRE(gt_rgb && gt_depth && depth && alpha && viewmat && n_out && workspace && status, "null buffers");
    QED_REQUIRE(capacity == 0 || (points && log_scale && colors), "null buffers");
    const long long nb = grow_blocks(height, width, stride);
    const long long need = (3 + 2 * kGrowWaves) * nb + kGrowTail;
    if (workspace_ints < need) {
        set_error("qed_depth_grow_candidates: workspace too small (%lld < %lld ints)", (long long)workspace_ints, need);
        return QED_E_WORKSPACE;
    }
    GrowArgs a;
    a.W = width; a.stride = stride; a.gw = (width + stride - 1) / stride;
    a.g = (long long)a.gw * ((height + stride - 1) / stride);
    a.depth_stride = depth_stride;
    a.fx = (double)fx; a.fy = (double)fy; a.cx = (double)cx; a.cy = (double)cy;
    a.hole_alpha = (double)hole_alpha; a.depth_tol = (double)depth_tol; a.depth_tol_rel = (double)depth_tol_rel;
    a.depth_min = (double)depth_min; a.depth_max = (double)depth_max; a.scale_factor = (double)scale_factor;
    a.capacity = capacity;
    const GrowPlanes s = {gt_rgb, gt_depth, depth, alpha, viewmat, mask};
    int* block_counts = workspace;
    int* block_offsets = workspace + nb;
    int* block_holes = workspace + 2 * nb;
    int* keep_words = workspace + 3 * nb;
    int* tail = workspace + (3 + 2 * kGrowWaves) * nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grow_count_kernel, dim3((unsigned)nb), dim3(kGrowThreads), 0, st, a, s, block_counts, block_holes,
                       keep_words);
    // (K <= height * width < 2^31: the scan never reports an overflow; its status word goes to the workspace)
    const int rc = qed_isect_scan(block_counts, (int)nb, block_offsets, tail, 0x7fffffffLL, tail + 4, stream);
    if (rc != QED_OK) return rc;
    hipLaunchKernelGGL(grow_write_kernel, dim3((unsigned)nb), dim3(kGrowThreads), 0, st, a, s, (int)nb,
                       (const int*)block_counts, (const int*)block_offsets, (const int*)block_holes,
                       (const int*)keep_words, (const int*)tail, points, log_scale, colors, n_out, status);
    return check_launch("qed_depth_grow_candidates");
}

extern "C" int qed_grow_append(int32_t n, int32_t k, const float* old_params, const float* old_exp_avg,
                               const float* old_exp_avg_sq, const int64_t* h_old_begin, const float* points,
                               const float* log_scale, const float* colors, float init_opacity, float* new_params,
                               float* new_exp_avg, float* new_exp_avg_sq, const int64_t* h_new_begin, void* stream) {
    QED_REQUIRE(n >= 0 && k >= 0 && (long long)n + k < (1ll << 30), "n, k out of range");
    QED_REQUIRE(h_old_begin && h_new_begin, "null layout");
    QED_REQUIRE(init_opacity > 0.f && init_opacity < 1.f, "init_opacity must lie in (0, 1)");
    const long long n_new = (long long)n + k;
    if (n_new == 0) return QED_OK;
    AppendArgs a = {};
    for (int g = 0; g < 6; ++g) {
        const long long w = (h_new_begin[g + 1] - h_new_begin[g]) / n_new;
        QED_REQUIRE(w * n_new == h_new_begin[g + 1] - h_new_begin[g], "new group sizes must be multiples of n + k");
        QED_REQUIRE(h_old_begin[g + 1] - h_old_begin[g] == w * n, "old group sizes must be width x n");
        a.L.width[g] = (int)w;
        a.L.total_width += (int)w;
    }
    QED_REQUIRE(h_old_begin[0] == 0 && h_new_begin[0] == 0, "the first group begins at 0");
    QED_REQUIRE(a.L.width[0] == 3 && a.L.width[1] == 3 && a.L.width[2] == 4 && a.L.width[3] == 1 && a.L.width[4] == 3 &&
                    a.L.width[5] % 3 == 0 && a.L.width[5] <= 45,
                "group order: means, scales, quats, opacities, features_dc, features_rest");
    for (int g = 0; g < 7; ++g) { a.L.old_begin[g] = h_old_begin[g]; a.L.new_begin[g] = h_new_begin[g]; }
    a.n = n; a.total = h_new_begin[6];
    a.sh_coeffs = a.L.width[5] / 3 + 1;
    a.opacity_logit = (float)log((double)init_opacity / (1.0 - (double)init_opacity));
    QED_REQUIRE(new_params && new_exp_avg && new_exp_avg_sq, "null buffers");
    QED_REQUIRE(n == 0 || (old_params && old_exp_avg && old_exp_avg_sq), "null buffers");
    QED_REQUIRE(k == 0 || (points && log_scale && colors), "null buffers");
    hipLaunchKernelGGL(grow_append_kernel, dim3(stream_grid((a.total + 3) / 4)), dim3(kGrowThreads), 0,
                       (hipStream_t)stream, a, old_params, old_exp_avg, old_exp_avg_sq, points, log_scale, colors,
                       new_params, new_exp_avg, new_exp_avg_sq);
    return check_launch("qed_grow_append");
}
