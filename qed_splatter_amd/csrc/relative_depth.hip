// Relative-depth supervision: Pearson, patch-wise Pearson and scale-and-shift aligned L1 between the rendered depth and a prior
// known up to scale and shift (a monocular network's depth or inverse depth).  include/qed_splat.h states every definition.
//
//   V = alpha > 0 & m != 0 & finite(d) & finite(g) & g > 0 (& d > 0 in inverse space); x = d or 1 / d.
//   Pearson        lambda (1 - rho) over V;  ScaleShiftL1  lambda mean |x - (s g + t)| with the least-squares s, t (constants);
//   PatchPearson   lambda mean over the contributing P x P boxes of (1 - rho_b).
//
// All three are functions of six raw moments of a set -- n, sum x, sum g, sum x^2, sum g^2, sum x g -- carried in DOUBLE from
// the float32 inputs and folded in a fixed order (qed_reduce.h; no floating-point atomics: the same input gives the same bits).
//   Pearson / ScaleShiftL1   the reduce pass streams the image once, a workgroup's six sums in its own slots of the workspace
//                            (at most kRdMaxGrid workgroups); ScaleShiftL1 streams once more for sum |r| (every workgroup folds
//                            the moments itself and forms s, t).  The gradient pass folds the same slots, once per workgroup,
//                            forms the coefficients once and multiplies per pixel.
//   PatchPearson             one workgroup per box (a wave per box for P <= 16) leaves the box's moments AND the coefficients
//                            of its gradient in the box's row of a table behind the slots; a one-workgroup launch folds the
//                            rows (B, sum (1 - rho_b), the whole image's moments) in box order.  The gradient pass reads its
//                            pixel's row.
// The per-pixel arithmetic is double as well: the bracket of the Pearson gradient, (g - mean g) - rho sqrt(vg / vx) (x - mean x),
// is a difference of nearly equal terms when rho is near 1, and sign(r) of a float32 residual would disagree with the float64
// reference near zero.  The passes stay bandwidth-bound (four float planes, the depth plane possibly strided by 4).
#include "qed_common.h"

namespace qed {

constexpr int kRdCols = 8;            // n | sum x | sum g | sum x^2 | sum g^2 | sum x g | sum |r| or sum (1 - rho_b) | B
constexpr int kRdMaxGrid = 512;       // workgroups of a streaming reduce launch = partials per column (two rounds of a fold)
constexpr int kRdRow = QED_RD_BOX_DOUBLES;   // a box's row: the six moments | contributes | mean x | mean g | c1 | c2 | rho_b
constexpr double kRdDegenerate = 1e-12;
static_assert(QED_RD_WS_HEAD_DOUBLES == kRdCols * kRdMaxGrid, "the slots of the streaming passes");
static_assert(kRdRow >= 12, "a box's row");

struct RdImage {
    int H, W;
    const float* depth; int depth_stride;                     // d(p) = depth[p * depth_stride]
    const float* alpha;
    const float* prior;
    const float* mask;                                        // may be NULL
    int inverse;
};

// One pixel: false outside V; else x, g and dx / dd in double.
__device__ __forceinline__ bool rd_load(const RdImage& im, size_t p, double* x, double* g, double* dxdd) {
    const float d = im.depth[p * (size_t)im.depth_stride];
    const float a = im.alpha[p], gf = im.prior[p];
    const float m = im.mask != nullptr ? im.mask[p] : 1.f;
    const bool ok = a > 0.f && m != 0.f && isfinite(d) && isfinite(gf) && gf > 0.f && (!im.inverse || d > 0.f);
    if (!ok) return false;
    *g = (double)gf;
    if (im.inverse) { const double inv = 1.0 / (double)d; *x = inv; *dxdd = -inv * inv; }
    else { *x = (double)d; *dxdd = 1.0; }
    return true;
}

__device__ __forceinline__ void rd_add(double* acc, double x, double g) {
    acc[0] += 1.0; acc[1] += x; acc[2] += g; acc[3] += x * x; acc[4] += g * g; acc[5] += x * g;
}

// What a set's six raw sums say.  A degenerate set (n < 2, or a variance within 1e-12 of its mean square) has ok = false and
// every figure 0.
struct RdMoments {
    double n, mx, mg, vx, vg, rho, s, t;
    bool ok;
};

__device__ __forceinline__ RdMoments rd_moments(const double* s) {
    RdMoments m = {s[0], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (!(s[0] >= 2.0)) return m;
    const double inv = 1.0 / s[0];
    const double mx = s[1] * inv, mg = s[2] * inv, exx = s[3] * inv, egg = s[4] * inv;
    const double vx = exx - mx * mx, vg = egg - mg * mg, cov = s[5] * inv - mx * mg;
    if (!(vx > kRdDegenerate * exx && vg > kRdDegenerate * egg)) return m;
    m.mx = mx; m.mg = mg; m.vx = vx; m.vg = vg;
    m.rho = cov / sqrt(vx * vg);
    m.s = cov / vg;
    m.t = mx - m.s * mg;
    m.ok = true;
    return m;
}

// The fold of the first `cols` columns of the partials by one workgroup of 256 threads, in a fixed order: a thread adds the
// partials b = threadIdx.x, + 256, ... of a column, then the workgroup sum.  Columns from `cols` on come back 0.
__device__ __forceinline__ void rd_fold(int n_blocks, int cols, const double* __restrict__ partials, double (*s_w)[4],
                                        double* s) {
    double v[kRdCols];
#pragma unroll
    for (int c = 0; c < kRdCols; ++c) {
        v[c] = 0.0;
        if (c < cols)
            for (int b = threadIdx.x; b < n_blocks; b += 256) v[c] += partials[(size_t)c * kRdMaxGrid + b];
    }
    block_sum_d<kRdCols>(v, s_w, s);
}

__device__ __forceinline__ int rd_cols(int type) {
    return type == QED_RD_PEARSON ? 6 : (type == QED_RD_SCALE_SHIFT_L1 ? 7 : 8);
}

__device__ __forceinline__ void rd_write_out(int type, const double* s, double lambda, const float* __restrict__ loss_base,
                                             double* __restrict__ out, float* __restrict__ out_f) {
    const RdMoments m = rd_moments(s);
    double loss = 0.0, B = 0.0, mean_rho = 0.0;
    if (type == QED_RD_PEARSON) {
        if (m.ok) loss = lambda * (1.0 - m.rho);
    } else if (type == QED_RD_SCALE_SHIFT_L1) {
        if (m.ok) loss = lambda * (s[6] / m.n);
    } else {
        B = s[7];
        if (B > 0.0) { loss = lambda * (s[6] / B); mean_rho = 1.0 - s[6] / B; }
    }
    out[0] = loss; out[1] = s[0]; out[2] = m.rho; out[3] = m.s; out[4] = m.t; out[5] = B; out[6] = mean_rho; out[7] = 0.0;
    if (out_f != nullptr) {
        out_f[0] = (float)loss;
        out_f[1] = (float)((loss_base != nullptr ? (double)loss_base[0] : 0.0) + loss);
    }
}

// ---- the streaming reduce pass (Pearson, ScaleShiftL1) -----------------------------------------------------------------------
__global__ void __launch_bounds__(256)
relative_depth_reduce_kernel(RdImage im, double* __restrict__ partials) {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t n_pix = (size_t)im.H * im.W;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += (size_t)gridDim.x * 256) {
        double x, g, dxdd;
        if (rd_load(im, p, &x, &g, &dxdd)) rd_add(acc, x, g);
    }
    __shared__ double s_w[6][4];
    __shared__ double s[6];
    block_sum_d<6>(acc, s_w, s);
    if (threadIdx.x < 6) partials[(size_t)threadIdx.x * kRdMaxGrid + blockIdx.x] = s[threadIdx.x];
}

// ScaleShiftL1's second stream: sum over V of |x - (s g + t)|, a workgroup's sum in its slot of column 6.
__global__ void __launch_bounds__(256)
relative_depth_residual_kernel(RdImage im, int n_blocks, double* __restrict__ partials) {
    __shared__ double s_w[kRdCols][4];
    __shared__ double s[kRdCols];
    rd_fold(n_blocks, 6, partials, s_w, s);
    const RdMoments m = rd_moments(s);
    double acc[1] = {0.0};
    const size_t n_pix = (size_t)im.H * im.W;
    if (m.ok) {
        for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += (size_t)gridDim.x * 256) {
            double x, g, dxdd;
            if (rd_load(im, p, &x, &g, &dxdd)) acc[0] += fabs(x - (m.s * g + m.t));
        }
    }
    __shared__ double r_w[1][4];
    __shared__ double r[1];
    block_sum_d<1>(acc, r_w, r);
    if (threadIdx.x == 0) partials[(size_t)6 * kRdMaxGrid + blockIdx.x] = r[0];
}

__global__ void __launch_bounds__(256)
relative_depth_finalize_kernel(int type, int n_blocks, const double* __restrict__ partials, double lambda,
                               const float* __restrict__ loss_base, double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kRdCols][4];
    __shared__ double s[kRdCols];
    rd_fold(n_blocks, rd_cols(type), partials, s_w, s);
    if (threadIdx.x == 0) rd_write_out(type, s, lambda, loss_base, out, out_f);
}

// ---- the box table (PatchPearson) --------------------------------------------------------------------------------------------
struct RdBoxes {
    int log2p, ox, oy, nbx, n_boxes;
    double min_count;                                         // K
};

// A box's row from its six sums: the moments, whether it contributes, and the coefficients of its gradient.
__device__ __forceinline__ void rd_write_row(double* __restrict__ row, const double* s, double min_count) {
    const RdMoments m = rd_moments(s);
    const bool on = m.ok && s[0] >= min_count;
#pragma unroll
    for (int c = 0; c < 6; ++c) row[c] = s[c];
    row[6] = on ? 1.0 : 0.0;
    row[7] = m.mx; row[8] = m.mg;
    row[9] = on ? 1.0 / (m.n * sqrt(m.vx * m.vg)) : 0.0;
    row[10] = on ? m.rho * sqrt(m.vg / m.vx) : 0.0;
    row[11] = on ? m.rho : 0.0;
}

// Small boxes (P <= 16, at most four pixels per lane): a WAVE per box, four boxes per workgroup -- no barrier, no LDS; the
// xor butterfly leaves the same bits in every lane.  With a workgroup per box three of four waves of a P = 8 box sat idle.
__global__ void __launch_bounds__(256)
relative_depth_box_wave_kernel(RdImage im, RdBoxes bx, double* __restrict__ table) {
    const int box = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (box >= bx.n_boxes) return;                            // (whole waves leave; nothing below synchronises)
    const int by = box / bx.nbx, bxi = box - by * bx.nbx;
    const int P = 1 << bx.log2p, i0 = by * P - bx.oy, j0 = bxi * P - bx.ox;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x & 63; t < P * P; t += 64) {
        const int i = i0 + (t >> bx.log2p), j = j0 + (t & (P - 1));
        if (i < 0 || i >= im.H || j < 0 || j >= im.W) continue;
        double x, g, dxdd;
        if (rd_load(im, (size_t)i * im.W + j, &x, &g, &dxdd)) rd_add(acc, x, g);
    }
    double s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = wave_sum_d(acc[c]);
    if ((threadIdx.x & 63) == 0) rd_write_row(table + (size_t)box * kRdRow, s, bx.min_count);
}

// Larger boxes: one workgroup per box, the box's pixels in row-major order over its threads.
template <int NT>
__global__ void __launch_bounds__(NT)
relative_depth_box_kernel(RdImage im, RdBoxes bx, double* __restrict__ table) {
    const int box = blockIdx.x, by = box / bx.nbx, bxi = box - by * bx.nbx;
    const int P = 1 << bx.log2p, i0 = by * P - bx.oy, j0 = bxi * P - bx.ox;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < P * P; t += NT) {
        const int i = i0 + (t >> bx.log2p), j = j0 + (t & (P - 1));
        if (i < 0 || i >= im.H || j < 0 || j >= im.W) continue;
        double x, g, dxdd;
        if (rd_load(im, (size_t)i * im.W + j, &x, &g, &dxdd)) rd_add(acc, x, g);
    }
    __shared__ double s_w[6][NT / 64];
    __shared__ double s[6];
    block_sum_d<6, NT>(acc, s_w, s);
    if (threadIdx.x == 0) rd_write_row(table + (size_t)box * kRdRow, s, bx.min_count);
}

// The rows folded in box order by one workgroup: the whole image's moments, sum (1 - rho_b) and B, left as ONE partial per
// column (the gradient pass folds them like any other), and the values.
__global__ void __launch_bounds__(256)
relative_depth_box_fold_kernel(int n_boxes, const double* __restrict__ table, double* __restrict__ partials, double lambda,
                               const float* __restrict__ loss_base, double* __restrict__ out, float* __restrict__ out_f) {
    double v[kRdCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_boxes; b += 256) {
        const double* row = table + (size_t)b * kRdRow;
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] += row[c];
        if (row[6] != 0.0) { v[6] += 1.0 - row[11]; v[7] += 1.0; }
    }
    __shared__ double s_w[kRdCols][4];
    __shared__ double s[kRdCols];
    block_sum_d<kRdCols>(v, s_w, s);
    if (threadIdx.x < kRdCols) partials[(size_t)threadIdx.x * kRdMaxGrid] = s[threadIdx.x];
    if (threadIdx.x == 0 && out != nullptr) rd_write_out(QED_RD_PATCH_PEARSON, s, lambda, loss_base, out, out_f);
}

// ---- the gradient pass -------------------------------------------------------------------------------------------------------
template <int TYPE>
__global__ void __launch_bounds__(256)
relative_depth_grad_kernel(RdImage im, RdBoxes bx, int n_blocks, const double* __restrict__ ws, double lambda,
                           const float* __restrict__ g_up, const float* __restrict__ loss_base, float* __restrict__ v_depth,
                           int v_depth_stride, int accumulate, double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kRdCols][4];
    __shared__ double s[kRdCols];
    rd_fold(n_blocks, rd_cols(TYPE), ws, s_w, s);
    if (out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)     // (both passes in one call: no fold launch in between)
        rd_write_out(TYPE, s, lambda, loss_base, out, out_f);
    // the fully scaled coefficients, once per workgroup
    const double up = (g_up != nullptr ? (double)g_up[0] : 1.0) * lambda;
    const RdMoments m = rd_moments(s);
    bool live;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (TYPE == QED_RD_PEARSON) {
        live = m.ok;
        if (live) { c1 = -up / (m.n * sqrt(m.vx * m.vg)); c2 = m.rho * sqrt(m.vg / m.vx); }
    } else if (TYPE == QED_RD_SCALE_SHIFT_L1) {
        live = m.ok;
        if (live) c0 = up / m.n;
    } else {
        live = s[7] > 0.0;
        if (live) c0 = -up / s[7];
    }
    const double* table = ws + QED_RD_WS_HEAD_DOUBLES;
    const size_t n_pix = (size_t)im.H * im.W;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += (size_t)gridDim.x * 256) {
        double x, g, dxdd;
        float val = 0.f;
        if (live && rd_load(im, p, &x, &g, &dxdd)) {
            if (TYPE == QED_RD_PEARSON) {
                val = (float)(c1 * ((g - m.mg) - c2 * (x - m.mx)) * dxdd);
            } else if (TYPE == QED_RD_SCALE_SHIFT_L1) {
                const double r = x - (m.s * g + m.t);
                val = (float)(c0 * (r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0)) * dxdd);
            } else {
                const int i = (int)(p / (size_t)im.W), j = (int)(p - (size_t)i * im.W);
                const double* row = table + ((size_t)((i + bx.oy) >> bx.log2p) * bx.nbx + ((j + bx.ox) >> bx.log2p)) * kRdRow;
                if (row[6] != 0.0) val = (float)(c0 * row[9] * ((g - row[8]) - row[10] * (x - row[7])) * dxdd);
            }
        }
        float* dst = v_depth + p * (size_t)v_depth_stride;
        if (!accumulate) *dst = val;
        else if (val != 0.f) *dst += val;
    }
}

}  // namespace qed

using namespace qed;

extern "C" int qed_relative_depth_loss(int32_t height, int32_t width, const float* depth, int32_t depth_stride,
                                       const float* alpha, const float* prior, const float* mask, int32_t type, float lambda,
                                       int32_t patch, int32_t offset_x, int32_t offset_y, float min_valid, uint32_t flags,
                                       const float* g_up, const float* loss_base, double* workspace, float* v_depth,
                                       int32_t v_depth_stride, double* out, float* out_f, void* stream) {
    const int reduce = (flags & QED_RD_REDUCE) != 0, grad = (flags & QED_RD_GRAD) != 0;
    const bool boxes = type == QED_RD_PATCH_PEARSON;
    QED_REQUIRE(height >= 0 && width >= 0, "negative size");
    QED_REQUIRE((flags & ~(uint32_t)(QED_RD_INVERSE | QED_RD_REDUCE | QED_RD_GRAD | QED_RD_ACCUMULATE)) == 0, "unknown flag");
    QED_REQUIRE(reduce || grad, "flags: QED_RD_REDUCE, QED_RD_GRAD or both");
    QED_REQUIRE(type == QED_RD_PEARSON || type == QED_RD_PATCH_PEARSON || type == QED_RD_SCALE_SHIFT_L1,
                "unknown relative depth loss type");
    QED_REQUIRE(lambda >= 0.f && lambda <= 3.4e38f, "lambda must be a finite number >= 0");
    int log2p = 0;
    if (boxes) {
        QED_REQUIRE(patch == 8 || patch == 16 || patch == 32 || patch == 64 || patch == 128,
                    "patch must be 8, 16, 32, 64 or 128");
        QED_REQUIRE(offset_x >= 0 && offset_x < patch && offset_y >= 0 && offset_y < patch, "offsets must lie in [0, patch)");
        QED_REQUIRE(min_valid > 0.f && min_valid <= 1.f, "min_valid must lie in (0, 1]");
        while ((1 << log2p) < patch) ++log2p;
    }
    QED_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7) == 0, "workspace: doubles");
    QED_REQUIRE(!reduce || (out != nullptr && ((uintptr_t)out & 7) == 0), "out: 8 doubles");
    QED_REQUIRE(out == nullptr || ((uintptr_t)out & 7) == 0, "out: 8 doubles");
    const long long n_pix = (long long)height * width;
    QED_REQUIRE(n_pix <= 0x7fffffffLL, "image too large");
    if (n_pix > 0) {
        QED_REQUIRE(depth != nullptr && depth_stride >= 1, "null depth");
        QED_REQUIRE(alpha != nullptr && prior != nullptr, "null alpha or prior");
        QED_REQUIRE(!grad || (v_depth != nullptr && v_depth_stride >= 1), "null output");
    }
    hipStream_t st = (hipStream_t)stream;
    RdImage im;
    im.H = height; im.W = width;
    im.depth = depth; im.depth_stride = depth_stride;
    im.alpha = alpha; im.prior = prior; im.mask = mask;
    im.inverse = (flags & QED_RD_INVERSE) != 0;
    RdBoxes bx = {0, 0, 0, 1, 0, 0.0};
    if (boxes && n_pix > 0) {
        bx.log2p = log2p; bx.ox = offset_x; bx.oy = offset_y;
        bx.nbx = (width - 1 + offset_x) / patch + 1;
        bx.n_boxes = bx.nbx * ((height - 1 + offset_y) / patch + 1);
        bx.min_count = std::max(2.0, std::ceil((double)min_valid * patch * patch));
    }
    // (the grids are functions of the size alone: a gradient pass in a later call folds the same slots)
    const unsigned grid = n_pix == 0 ? 0u : stream_grid(n_pix, kRdMaxGrid);
    const unsigned grad_grid = stream_grid(n_pix, 2048);
    const int n_partials = boxes ? 1 : (int)grid;
    double* table = workspace + QED_RD_WS_HEAD_DOUBLES;
    if (reduce) {
        if (boxes) {
            if (bx.n_boxes > 0) {
                if (patch <= 16)
                    hipLaunchKernelGGL(relative_depth_box_wave_kernel, dim3((bx.n_boxes + 3) / 4), dim3(256), 0, st, im, bx,
                                       table);
                else
                    hipLaunchKernelGGL(relative_depth_box_kernel<1024>, dim3(bx.n_boxes), dim3(1024), 0, st, im, bx, table);
            }
            hipLaunchKernelGGL(relative_depth_box_fold_kernel, dim3(1), dim3(256), 0, st, bx.n_boxes, (const double*)table,
                               workspace, (double)lambda, loss_base, out, out_f);
        } else {
            if (grid > 0) {
                hipLaunchKernelGGL(relative_depth_reduce_kernel, dim3(grid), dim3(256), 0, st, im, workspace);
                if (type == QED_RD_SCALE_SHIFT_L1)
                    hipLaunchKernelGGL(relative_depth_residual_kernel, dim3(grid), dim3(256), 0, st, im, (int)grid, workspace);
            }
            if (!grad || grid == 0)
                hipLaunchKernelGGL(relative_depth_finalize_kernel, dim3(1), dim3(256), 0, st, (int)type, (int)grid,
                                   (const double*)workspace, (double)lambda, loss_base, out, out_f);
        }
    }
    if (grad && n_pix > 0) {
        auto kernel = type == QED_RD_PEARSON ? relative_depth_grad_kernel<QED_RD_PEARSON>
                      : (type == QED_RD_SCALE_SHIFT_L1 ? relative_depth_grad_kernel<QED_RD_SCALE_SHIFT_L1>
                                                       : relative_depth_grad_kernel<QED_RD_PATCH_PEARSON>);
        const bool writes_out = reduce && !boxes;
        hipLaunchKernelGGL(kernel, dim3(grad_grid), dim3(256), 0, st, im, bx, n_partials, (const double*)workspace,
                           (double)lambda, g_up, loss_base, v_depth, v_depth_stride, (int)((flags & QED_RD_ACCUMULATE) != 0),
                           writes_out ? out : nullptr, writes_out ? out_f : nullptr);
    }
    return check_launch("qed_relative_depth_loss");
}
