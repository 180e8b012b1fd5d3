// Normal consistency and normal smoothness in training: the two regularisers on the rendered normal that need no sensor
// normals, with the backward pass of the depth stencil.  include/qed_splat.h states every definition.
//
//   consistency   lambda_c * mean over V_c of (1 - n^ . N): the rendered normal n^ = A / |A| against the normal N of the
//                 RENDERED depth z = D / alpha (qed_normal_maps' stencil, bit for bit the same decisions), so gradients reach
//                 A at the pixel and z at its four neighbours -- and from z the accumulated depth D and alpha.
//   smoothness    lambda_tv * [mean over E_x and the channels of |n^(p + x) - n^(p)| + the same over E_y]: gradients reach A.
//
// Two passes over the image, each one pixel per thread with its neighbours read through the caches:
//   the reduce pass  per pixel its own stencil and its right and lower neighbour pair; the workgroup's six sums as doubles,
//                    folded by a one-workgroup launch in a fixed order (qed_reduce.h): no floating-point atomics, the same
//                    input gives the same bits.
//   the gradient pass  reads the three denominators from device memory (they never reach the host) and GATHERS: the depth
//                    gradient of pixel q is the sum, in a fixed order, of what the stencils centred on q's four neighbours
//                    hand to q, each re-evaluated from the radius-2 diamond of z around q (13 depths); no scatter, no atomics,
//                    no intermediate image.  (The alternative -- a first pass that leaves d l / d (dx), d l / d (dy) per pixel,
//                    six values, and a second that reads four neighbours -- moves 48 B per pixel more through memory to save
//                    four stencil evaluations per pixel; it was not built.  Measured (profiles/normal_consistency.txt): 158 us
//                    at 1080p for 83 MB, so the gather is bound by its f64 arithmetic -- ~80 divisions per pixel --, not its bytes.)
// The per-pixel arithmetic is double from the float32 inputs, as in qed_normal_maps / qed_normal_loss.
//
//   qed_normal_rows_merge_depth   qed_normal_rows_merge with slot 11 (depth): the rows of a 4-channel normal pass.
#include "qed_common.h"

namespace qed {

constexpr int kNcCols = 6;     // sum of 1 - n^ . N | |V_c| | sum over E_x of |dn| | |E_x| | sum over E_y of |dn| | |E_y|
constexpr int kNcMaxGrid = QED_NORMAL_CONSISTENCY_WS_DOUBLES / kNcCols;

struct NcImage {
    int H, W;
    const float* accum; int accum_stride;                     // A(p) = accum[p * accum_stride + 0..2]
    const float* alpha;
    const float* depth; int depth_stride;
    const float* mask;                                        // may be NULL
    double fx, fy, cx, cy;
    float min_alpha;
};

// qed_normal_maps' surface depth: z = D / alpha where alpha >= min_alpha; finite and > 0, else NaN.  Outside the image: NaN.
__device__ __forceinline__ double nc_depth(const NcImage& im, int x, int y) {
    if (x < 0 || y < 0 || x >= im.W || y >= im.H) return __builtin_nan("");
    const size_t p = (size_t)y * im.W + x;
    const float a = im.alpha[p];
    if (!(a >= im.min_alpha)) return __builtin_nan("");
    const double z = (double)im.depth[p * (size_t)im.depth_stride] / (double)a;
    return (isfinite(z) && z > 0.0) ? z : __builtin_nan("");
}

// n^ = A / |A| where alpha >= min_alpha and |A| > 1e-8 (n, 1 / |A|); `counts`: n^ defined AND the mask non-zero
__device__ __forceinline__ bool nc_normal(const NcImage& im, int x, int y, double* n, double* inv_len) {
    n[0] = n[1] = n[2] = 0.0;
    *inv_len = 0.0;
    if (x < 0 || y < 0 || x >= im.W || y >= im.H) return false;
    const size_t p = (size_t)y * im.W + x;
    const float* A = im.accum + p * (size_t)im.accum_stride;
    const double A0 = A[0], A1 = A[1], A2 = A[2];
    const float a = im.alpha[p];
    const bool m = im.mask == nullptr || im.mask[p] != 0.f;
    const double len = sqrt(A0 * A0 + A1 * A1 + A2 * A2);
    if (!(a >= im.min_alpha && len > 1e-8 && m)) return false;
    const double il = 1.0 / len;
    n[0] = A0 * il; n[1] = A1 * il; n[2] = A2 * il;
    *inv_len = il;
    return true;
}

// The stencil centred on (x, y) from its four neighbours' depths (and the centre's, for validity only): N, |dy x dx|, dx, dy.
__device__ __forceinline__ bool nc_stencil(const NcImage& im, int x, int y, double zc, double zl, double zr, double zu,
                                           double zd, double* N, double* len_out, double* dx, double* dy) {
    if (!(x > 0 && y > 0 && x < im.W - 1 && y < im.H - 1)) return false;
    if (isnan(zc) || isnan(zl) || isnan(zr) || isnan(zu) || isnan(zd)) return false;
    const double ul = ((double)(x - 1) + 0.5 - im.cx) / im.fx, ur = ((double)(x + 1) + 0.5 - im.cx) / im.fx;
    const double uc = ((double)x + 0.5 - im.cx) / im.fx;
    const double vu = ((double)(y - 1) + 0.5 - im.cy) / im.fy, vd = ((double)(y + 1) + 0.5 - im.cy) / im.fy;
    const double vc = ((double)y + 0.5 - im.cy) / im.fy;
    dx[0] = ur * zr - ul * zl; dx[1] = vc * zr - vc * zl; dx[2] = zr - zl;
    dy[0] = uc * zd - uc * zu; dy[1] = vd * zd - vu * zu; dy[2] = zd - zu;
    const double cr[3] = {dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]};
    const double len = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    if (!(len > 1e-20)) return false;
    N[0] = cr[0] / len; N[1] = cr[1] / len; N[2] = cr[2] / len;
    *len_out = len;
    return true;
}

__device__ __forceinline__ double nc_triple(const double* g, const double* a, const double* b) {       // g . (a x b)
    return g[0] * (a[1] * b[2] - a[2] * b[1]) + g[1] * (a[2] * b[0] - a[0] * b[2]) + g[2] * (a[0] * b[1] - a[1] * b[0]);
}

__device__ __forceinline__ double nc_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

// ---- the reduce pass ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
normal_consistency_reduce_kernel(NcImage im, int do_c, int do_tv, double* __restrict__ partials) {
    double acc[kNcCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t n_pix = (size_t)im.H * im.W;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += stride) {     // (in index order per thread)
        const int y = (int)(p / im.W), x = (int)(p - (size_t)y * im.W);
        double n[3], il;
        const bool ok = nc_normal(im, x, y, n, &il);
        if (!ok) continue;                                    // every term of this pixel needs its own n^ and mask
        if (do_c) {
            double N[3], len, dx[3], dy[3];
            if (nc_stencil(im, x, y, nc_depth(im, x, y), nc_depth(im, x - 1, y), nc_depth(im, x + 1, y),
                           nc_depth(im, x, y - 1), nc_depth(im, x, y + 1), N, &len, dx, dy)) {
                acc[0] += 1.0 - (n[0] * N[0] + n[1] * N[1] + n[2] * N[2]);
                acc[1] += 1.0;
            }
        }
        if (do_tv) {
            double m[3], ml;
            if (nc_normal(im, x + 1, y, m, &ml)) {
                acc[2] += fabs(m[0] - n[0]) + fabs(m[1] - n[1]) + fabs(m[2] - n[2]);
                acc[3] += 1.0;
            }
            if (nc_normal(im, x, y + 1, m, &ml)) {
                acc[4] += fabs(m[0] - n[0]) + fabs(m[1] - n[1]) + fabs(m[2] - n[2]);
                acc[5] += 1.0;
            }
        }
    }
    __shared__ double s_w[kNcCols][4];
    __shared__ double s[kNcCols];
    block_sum_d(acc, s_w, s);
    if (threadIdx.x < kNcCols) partials[(size_t)threadIdx.x * kNcMaxGrid + blockIdx.x] = s[threadIdx.x];
}

__global__ void __launch_bounds__(256)
normal_consistency_finalize_kernel(int n_blocks, const double* __restrict__ partials, double lambda_c, double lambda_tv,
                                   double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kNcCols][4];
    __shared__ double s[kNcCols];
    double v[kNcCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int blk = threadIdx.x; blk < n_blocks; blk += 256) {
#pragma unroll
        for (int c = 0; c < kNcCols; ++c) v[c] += partials[(size_t)c * kNcMaxGrid + blk];
    }
    block_sum_d(v, s_w, s);
    if (threadIdx.x == 0) {                                   // (an empty set: its sum is 0, and so is its mean)
        const double mean_c = s[0] / (s[1] > 0.0 ? s[1] : 1.0);
        const double mean_x = s[2] / (3.0 * (s[3] > 0.0 ? s[3] : 1.0));
        const double mean_y = s[4] / (3.0 * (s[5] > 0.0 ? s[5] : 1.0));
        out[0] = lambda_c * mean_c; out[1] = mean_c; out[2] = s[1];
        out[3] = lambda_tv * (mean_x + mean_y); out[4] = mean_x; out[5] = mean_y; out[6] = s[3]; out[7] = s[5];
        if (out_f != nullptr) { out_f[0] = (float)out[0]; out_f[1] = (float)out[3]; }
    }
}

// ---- the gradient pass -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
normal_consistency_grad_kernel(NcImage im, int do_c, int do_tv, double lambda_c, double lambda_tv,
                               const float* __restrict__ g_c, const float* __restrict__ g_tv,
                               const float* __restrict__ nl_v_accum, const float* __restrict__ nl_scale,
                               const float* __restrict__ g_nl, const double* __restrict__ sums,
                               float* __restrict__ v_accum, int v_accum_stride, float* __restrict__ v_depth,
                               int v_depth_stride, float* __restrict__ v_alpha) {
    const size_t n_pix = (size_t)im.H * im.W;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_pix) return;
    const int y = (int)(q / im.W), x = (int)(q - (size_t)y * im.W);
    // the fully scaled weights: upstream gradient * lambda / max(count, 1), the counts read from the reduce pass's result
    const double cnt_c = sums[2], cnt_x = sums[6], cnt_y = sums[7];
    const double wc = do_c ? (g_c != nullptr ? (double)g_c[0] : 1.0) * lambda_c / (cnt_c > 0.0 ? cnt_c : 1.0) : 0.0;
    const double gtv = do_tv ? (g_tv != nullptr ? (double)g_tv[0] : 1.0) * lambda_tv : 0.0;
    const double wx = gtv / (3.0 * (cnt_x > 0.0 ? cnt_x : 1.0)), wy = gtv / (3.0 * (cnt_y > 0.0 ? cnt_y : 1.0));

    // the rendered normal here and at the four neighbours: index 0 = q, 1 = left, 2 = right, 3 = up, 4 = down
    const int ox[5] = {0, -1, 1, 0, 0}, oy[5] = {0, 0, 0, -1, 1};
    double n[5][3], il[5];
    bool ok[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ok[i] = nc_normal(im, x + ox[i], y + oy[i], n[i], &il[i]);

    double vn[3] = {0.0, 0.0, 0.0};                           // d loss / d n^(q)
    double vz = 0.0;                                          // d loss / d z(q)
    double zq = __builtin_nan("");
    if (do_c) {
        // the radius-2 diamond of z around q: z[dy + 2][dx + 2]
        double z[5][5];
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                if ((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx) <= 2) z[dy + 2][dx + 2] = nc_depth(im, x + dx, y + dy);
            }
        }
        zq = z[2][2];
        const double e[3] = {((double)x + 0.5 - im.cx) / im.fx, ((double)y + 0.5 - im.cy) / im.fy, 1.0};
#pragma unroll
        for (int i = 0; i < 5; ++i) {                         // (a fixed order: the sum's bits do not depend on the run)
            if (!ok[i]) continue;                             // the stencil's pixel is in V_c only with its n^ and mask
            const int sx = 2 + ox[i], sy = 2 + oy[i];
            double N[3], len, dx[3], dy[3];
            if (!nc_stencil(im, x + ox[i], y + oy[i], z[sy][sx], z[sy][sx - 1], z[sy][sx + 1], z[sy - 1][sx], z[sy + 1][sx],
                            N, &len, dx, dy))
                continue;
            if (i == 0) {                                     // q's own stencil: d (1 - n^ . N) / d n^ = -N
                vn[0] -= wc * N[0]; vn[1] -= wc * N[1]; vn[2] -= wc * N[2];
                continue;
            }
            // d l / d (dy x dx) of l = wc (1 - n^ . N): (I - N N^T) (-wc n^) / |dy x dx|
            const double nN = n[i][0] * N[0] + n[i][1] * N[1] + n[i][2] * N[2];
            const double G[3] = {-wc * (n[i][0] - N[0] * nN) / len, -wc * (n[i][1] - N[1] * nN) / len,
                                 -wc * (n[i][2] - N[2] * nN) / len};
            // q is that stencil's right (i == 1), left (2), lower (3) or upper (4) neighbour:
            //   d dx / d z_right = e_q, d dx / d z_left = -e_q, d dy / d z_down = e_q, d dy / d z_up = -e_q
            if (i == 1) vz += nc_triple(G, dy, e);
            else if (i == 2) vz -= nc_triple(G, dy, e);
            else if (i == 3) vz += nc_triple(G, e, dx);
            else vz -= nc_triple(G, e, dx);
        }
    }
    if (do_tv && ok[0]) {
#pragma unroll
        for (int i = 1; i < 5; ++i) {
            if (!ok[i]) continue;
            const double w = i < 3 ? wx : wy;
#pragma unroll
            for (int k = 0; k < 3; ++k) vn[k] += w * nc_sign(n[0][k] - n[i][k]);
        }
    }
    double vA[3] = {0.0, 0.0, 0.0};
    if (ok[0]) {
        const double nv = n[0][0] * vn[0] + n[0][1] * vn[1] + n[0][2] * vn[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) vA[k] = (vn[k] - n[0][k] * nv) * il[0];
    }
    if (nl_v_accum != nullptr) {                              // qed_normal_loss' unscaled image joins here
        const double s = (double)nl_scale[0] * (g_nl != nullptr ? (double)g_nl[0] : 1.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) vA[k] += s * (double)nl_v_accum[3 * q + k];
    }
    float* va = v_accum + q * (size_t)v_accum_stride;
    va[0] = (float)vA[0]; va[1] = (float)vA[1]; va[2] = (float)vA[2];
    float vd = 0.f, val = 0.f;
    if (do_c && !isnan(zq) && vz != 0.0) {                    // z = D / alpha: d z / d D = 1 / alpha, d z / d alpha = -z / alpha
        const double a = (double)im.alpha[q];
        vd = (float)(vz / a);
        val = (float)(-vz * zq / a);
    }
    if (v_depth != nullptr) v_depth[q * (size_t)v_depth_stride] = vd;
    if (v_alpha != nullptr) v_alpha[q] = val;
}

// ---- the rows of a 4-channel normal pass into the colour pass's rows -------------------------------------------------------------
__global__ void __launch_bounds__(256)
normal_rows_merge_depth_kernel(long long total, const float4* __restrict__ normal_rows, const float* __restrict__ scale,
                               float4* __restrict__ rows) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= total) return;
    const float4 a0 = normal_rows[4 * r], a1 = normal_rows[4 * r + 1], a2 = normal_rows[4 * r + 2];
    float4 d0 = rows[4 * r], d1 = rows[4 * r + 1], d2 = rows[4 * r + 2];
    const float s = scale != nullptr ? scale[0] : 1.f;
    d0.x += s * a0.x; d0.y += s * a0.y;                       // 2-D mean; slots 2, 3 (absgrad) are written back as read
    d1.x += s * a1.x; d1.y += s * a1.y; d1.z += s * a1.z; d1.w += s * a1.w;      // conic a, b, c | opacity
    d2.w += s * a2.w;                                         // depth; slots 8..10 (colour) are written back as read
    rows[4 * r] = d0;
    rows[4 * r + 1] = d1;
    rows[4 * r + 2] = d2;
}

}  // namespace qed

using namespace qed;

extern "C" int qed_normal_consistency(int32_t height, int32_t width, const float* accum, int32_t accum_stride,
                                      const float* alpha, const float* depth, int32_t depth_stride, float fx, float fy,
                                      float cx, float cy, float min_alpha, const float* mask, float lambda_c, float lambda_tv,
                                      uint32_t flags, const float* g_c, const float* g_tv, const float* nl_v_accum,
                                      const float* nl_scale, const float* g_nl, double* workspace, float* v_accum,
                                      int32_t v_accum_stride, float* v_depth, int32_t v_depth_stride, float* v_alpha,
                                      double* out, float* out_f, void* stream) {
    const int do_c = (flags & QED_NC_CONSISTENCY) != 0, do_tv = (flags & QED_NC_TV) != 0;
    const int reduce = (flags & QED_NC_REDUCE) != 0, grad = (flags & QED_NC_GRAD) != 0;
    QED_REQUIRE(height >= 0 && width >= 0, "negative size");
    QED_REQUIRE((flags & ~(uint32_t)(QED_NC_CONSISTENCY | QED_NC_TV | QED_NC_REDUCE | QED_NC_GRAD)) == 0, "unknown flag");
    QED_REQUIRE(reduce || grad, "flags: QED_NC_REDUCE, QED_NC_GRAD or both");
    QED_REQUIRE(out != nullptr && ((uintptr_t)out & 7) == 0, "out: 8 doubles");
    QED_REQUIRE(!reduce || (workspace != nullptr && ((uintptr_t)workspace & 7) == 0), "workspace: doubles");
    const long long n_pix = (long long)height * width;
    QED_REQUIRE(n_pix <= 0x7fffffffLL, "image too large");
    if (n_pix > 0) {
        QED_REQUIRE(accum && alpha && accum_stride >= 3, "null input");
        QED_REQUIRE(!do_c || (depth != nullptr && depth_stride >= 1 && fx != 0.f && fy != 0.f),
                    "the consistency term needs the depth and non-zero focal lengths");
        QED_REQUIRE(!grad || (v_accum != nullptr && v_accum_stride >= 3 && (v_depth == nullptr || v_depth_stride >= 1)),
                    "null output");
        QED_REQUIRE(nl_v_accum == nullptr || nl_scale != nullptr, "the normal loss's image needs its scale");
    }
    hipStream_t st = (hipStream_t)stream;
    NcImage im;
    im.H = height; im.W = width;
    im.accum = accum; im.accum_stride = accum_stride;
    im.alpha = alpha;
    im.depth = depth; im.depth_stride = depth_stride;
    im.mask = mask;
    im.fx = (double)fx; im.fy = (double)fy; im.cx = (double)cx; im.cy = (double)cy;
    im.min_alpha = min_alpha;
    if (reduce) {
        const unsigned grid = n_pix == 0 ? 0u : stream_grid(n_pix, kNcMaxGrid);
        if (grid > 0)
            hipLaunchKernelGGL(normal_consistency_reduce_kernel, dim3(grid), dim3(256), 0, st, im, do_c, do_tv, workspace);
        hipLaunchKernelGGL(normal_consistency_finalize_kernel, dim3(1), dim3(256), 0, st, (int)grid,
                           (const double*)workspace, do_c ? (double)lambda_c : 0.0, do_tv ? (double)lambda_tv : 0.0, out,
                           out_f);
    }
    if (grad && n_pix > 0)
        hipLaunchKernelGGL(normal_consistency_grad_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, im, do_c,
                           do_tv, (double)lambda_c, (double)lambda_tv, g_c, g_tv, nl_v_accum, nl_scale, g_nl,
                           (const double*)out, v_accum, v_accum_stride, v_depth, v_depth_stride, v_alpha);
    return check_launch("qed_normal_consistency");
}

extern "C" int qed_normal_rows_merge_depth(int64_t total, const float* normal_rows, const float* scale, float* rows,
                                           void* stream) {
    QED_REQUIRE(total >= 0, "negative size");
    if (total == 0) return QED_OK;
    QED_REQUIRE(normal_rows && rows, "null pointer");
    QED_REQUIRE((((uintptr_t)normal_rows | (uintptr_t)rows) & 15) == 0, "rows must be 16-byte aligned");
    const long long grid = ((long long)total + 255) / 256;
    QED_REQUIRE(grid <= 0x7fffffffLL, "too many rows");
    hipLaunchKernelGGL(normal_rows_merge_depth_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                       (long long)total, (const float4*)normal_rows, scale, (float4*)rows);
    return check_launch("qed_normal_rows_merge_depth");
}
