// Robust depth losses and an edge-aware depth smoothness term in training.  include/qed_splat.h states every definition.
//
//   data term     depth_lambda * sum over V of w rho(|a - b|) / max(|V|, 1), a = d m, b = g m; V, the reference's validity, and
//                 the fix-up of d (alpha == 0 pixels take the channel's maximum) are those of loss.hip's depth-L1 term.
//   smoothness    tv_lambda * (E_x / max(N_x, 1) + E_y / max(N_y, 1)) over the neighbour pairs with alpha > 0, a finite d and a
//                 non-zero mask at both ends, optionally weighted by exp(-|colour difference|) of the ground-truth image.
//
// Two streaming passes, each a stream over at most seven float planes (depth, alpha, sensor depth, mask, three colours):
//   the reduce pass    per pixel its own data term and its right and lower pair; the workgroup's six sums as doubles in its
//                      own slots (qed_reduce.h), at most kDlMaxGrid workgroups.  No floating-point atomics.
//   the gradient pass  every workgroup folds those slots ITSELF, once, in a fixed order (the launch-boundary reduce: 12 KB out
//                      of L2 per workgroup instead of a one-workgroup launch in between), forms upstream * lambda / max(n, 1)
//                      ONCE and multiplies per pixel; a pixel's smoothness gradient is GATHERED from the up to four pairs it
//                      belongs to, in a fixed order.  Every output element is written; the same input gives the same bits.
// With both passes in one call (the fused step) that is two launches; the reduce pass alone is followed by a one-workgroup
// fold that leaves the values.  The per-pixel arithmetic is float32 (every decision -- validity, sign(a - b), alpha > 0 -- is
// an exact function of the float32 inputs; rho and the weights are a few ulp), the sums are carried in double.
#include "qed_common.h"

namespace qed {

constexpr int kDlCols = 6;            // sum of w rho | |V| | E_x | N_x | E_y | N_y
constexpr int kDlMaxGrid = 256;       // workgroups of the reduce pass = partials per column (one per thread of a fold)
constexpr int kDlReduceThreads = 1024;
constexpr int kDlReduceRows = kDlReduceThreads / 64, kDlGradRows = 4;      // tiles of 64 pixels x one row per wave
constexpr int kDlMaxSlot = 256;       // floats behind the partials: [0, 256) per-workgroup maxima, [256] the maximum in use
static_assert(QED_DEPTH_LOSS_WS_DOUBLES >= kDlCols * kDlMaxGrid + (kDlMaxSlot + 2) / 2, "workspace too small");

struct DlImage {
    int H, W;
    const float* depth; int depth_stride;                     // d(p) = depth[p * depth_stride]
    const float* alpha;                                       // may be NULL without the fix-up and the smoothness term
    const float* gt;                                          // sensor depth
    const float* mask;                                        // may be NULL
    const float* rgb;                                         // ground-truth colour [H,W,3]; NULL unless edge-aware
    int type;
    float delta, inv_delta;
    int fixup, data, tv, tv_edge;
};

__device__ __forceinline__ float dl_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// What the terms read of one pixel.  A pixel's neighbours are loaded UNCONDITIONALLY, at an index clamped to the image, before
// anything is decided: as load-then-branch rounds (is the pixel a pair's end? then load its neighbour, ...) the passes were
// bound by four to five dependent trips to memory per pixel, not by their bytes (profiles/depth_loss.txt).
struct DlSite {
    float d, alpha, m;
    float c[3];
};

template <bool RGB>
__device__ __forceinline__ DlSite dl_load(const DlImage& im, size_t p) {
    DlSite s;
    s.d = im.depth[p * (size_t)im.depth_stride];
    s.alpha = im.alpha != nullptr ? im.alpha[p] : 1.f;
    s.m = im.mask != nullptr ? im.mask[p] : 1.f;
    if constexpr (RGB) { s.c[0] = im.rgb[3 * p]; s.c[1] = im.rgb[3 * p + 1]; s.c[2] = im.rgb[3 * p + 2]; }
    else { s.c[0] = s.c[1] = s.c[2] = 0.f; }
    return s;
}

// mean over the channels of |I(q) - I(p)|
__device__ __forceinline__ float dl_cdiff(const DlSite& p, const DlSite& q) {
    return (fabsf(q.c[0] - p.c[0]) + fabsf(q.c[1] - p.c[1]) + fabsf(q.c[2] - p.c[2])) * (1.f / 3.f);
}

// a smoothness pair's end: alpha > 0, a finite depth, a non-zero mask
__device__ __forceinline__ bool dl_tv_ok(const DlSite& s) { return s.alpha > 0.f && isfinite(s.d) && s.m != 0.f; }

// The data term of a pixel with depth d (fixed up), sensor depth g and the colour differences gx, gy to its right and lower
// neighbour: false outside V; else w rho(r) and w rho'(r) sign(a - b) m.
__device__ __forceinline__ bool dl_data(const DlImage& im, float d, float m, float g, float gx, float gy, float* val,
                                        float* dval) {
    const float a = d * m, b = g * m;
    if (!(isfinite(a) && isfinite(b) && b > 0.f)) return false;
    const float diff = a - b, r = fabsf(diff);
    float rho, drho;
    switch (im.type) {
        case QED_DL_MSE: rho = r * r; drho = 2.f * r; break;
        case QED_DL_LOGL1:
        case QED_DL_EDGE_LOGL1: rho = log1pf(r); drho = 1.f / (1.f + r); break;
        case QED_DL_HUBER:
            if (r <= im.delta) { rho = r * r * (0.5f * im.inv_delta); drho = r * im.inv_delta; }
            else { rho = r - 0.5f * im.delta; drho = 1.f; }
            break;
        default: rho = r; drho = 1.f; break;
    }
    const float w = im.type == QED_DL_EDGE_LOGL1 ? 0.5f * (expf(-gx) + expf(-gy)) : 1.f;
    *val = w * rho;
    *dval = w * drho * dl_sign(diff) * m;
    return true;
}

// ---- the channel maximum, where the caller has none (loss.hip's post_max_kernel: the same fold) ---------------------------------
__global__ void __launch_bounds__(256)
depth_loss_max_kernel(int n_pix, const float* __restrict__ depth, int depth_stride, float* __restrict__ part) {
    float dmax = -3.0e38f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n_pix; i += (size_t)gridDim.x * 256)
        dmax = fmaxf(dmax, depth[i * (size_t)depth_stride]);
    dmax = wave_max(dmax);
    __shared__ float s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = dmax;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

// ---- the reduce pass ---------------------------------------------------------------------------------------------------------
// RGB: an edge-aware term reads the colour image; NEIGHBOURS: the right and lower neighbour are read (RGB or the smoothness term)
template <bool RGB, bool NEIGHBOURS>
__global__ void __launch_bounds__(kDlReduceThreads)
depth_loss_reduce_kernel(DlImage im, const float* __restrict__ dmax_in, int n_max_part, float* __restrict__ max_slots,
                         double* __restrict__ partials) {
    constexpr int NW = kDlReduceThreads / 64;
    __shared__ float s_m[NW];
    float dmax = 0.f;
    if (im.fixup) {
        if (dmax_in != nullptr) {
            dmax = dmax_in[0];
        } else {                                              // this call's own maxima (depth_loss_max_kernel)
            float dm = -3.0e38f;
            for (int b = threadIdx.x; b < n_max_part; b += kDlReduceThreads) dm = fmaxf(dm, max_slots[b]);
            dm = wave_max(dm);
            if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = dm;
            __syncthreads();
            dmax = s_m[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) dmax = fmaxf(dmax, s_m[w]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) max_slots[kDlMaxSlot] = dmax;

    double acc[kDlCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // a workgroup walks 64 x 16 tiles (a wave per row piece): a pixel's lower neighbour is mostly a load of this workgroup
    const int W = im.W, tiles_x = (im.W + 63) / 64, n_tiles = tiles_x * ((im.H + kDlReduceRows - 1) / kDlReduceRows);
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {       // (in tile order per thread)
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x = tx * 64 + lx, y = ty * kDlReduceRows + ly;
        if (x >= im.W || y >= im.H) continue;
        const size_t p = (size_t)y * W + x;
        const bool has_r = x < im.W - 1, has_d = y < im.H - 1;
        // every load of this pixel up front (a neighbour that does not exist: the pixel itself)
        const DlSite c = dl_load<RGB>(im, p);
        const DlSite r = NEIGHBOURS ? dl_load<RGB>(im, has_r ? p + 1 : p) : c;
        const DlSite dn = NEIGHBOURS ? dl_load<RGB>(im, has_d ? p + W : p) : c;
        const float g = im.data ? im.gt[p] : 0.f;
        const float gx = RGB && has_r ? dl_cdiff(c, r) : 0.f, gy = RGB && has_d ? dl_cdiff(c, dn) : 0.f;
        const float d = (im.fixup && !(c.alpha > 0.f)) ? dmax : c.d;            // loss.hip: p.a > 0.f ? d_render : dmax
        if (im.data) {
            float val, dval;
            if (dl_data(im, d, c.m, g, gx, gy, &val, &dval)) { acc[0] += (double)val; acc[1] += 1.0; }
        }
        if (im.tv && dl_tv_ok(c)) {
            if (has_r && dl_tv_ok(r)) { acc[2] += (double)((im.tv_edge ? expf(-gx) : 1.f) * fabsf(r.d - c.d)); acc[3] += 1.0; }
            if (has_d && dl_tv_ok(dn)) { acc[4] += (double)((im.tv_edge ? expf(-gy) : 1.f) * fabsf(dn.d - c.d)); acc[5] += 1.0; }
        }
    }
    __shared__ double s_w[kDlCols][NW];
    __shared__ double s[kDlCols];
    block_sum_d<kDlCols, kDlReduceThreads>(acc, s_w, s);
    if (threadIdx.x < kDlCols) partials[(size_t)threadIdx.x * kDlMaxGrid + blockIdx.x] = s[threadIdx.x];
}

// The fold of the reduce pass's partials by one workgroup of 256 threads, a partial per thread and column: s[0..5].
__device__ __forceinline__ void dl_fold(int n_blocks, const double* __restrict__ partials, double (*s_w)[4], double* s) {
    static_assert(kDlMaxGrid <= 256, "one partial per thread");
    double v[kDlCols];
    const bool ok = (int)threadIdx.x < n_blocks;
#pragma unroll
    for (int c = 0; c < kDlCols; ++c) v[c] = ok ? partials[(size_t)c * kDlMaxGrid + threadIdx.x] : 0.0;
    block_sum_d(v, s_w, s);
}

__device__ __forceinline__ double dl_at_least_one(double n) { return n > 0.0 ? n : 1.0; }

// (an empty set: its sum is 0, and so is its mean)
__device__ __forceinline__ void dl_write_out(const double* s, double lambda_d, double lambda_tv, float dmax,
                                             const float* __restrict__ loss_base, double* __restrict__ out,
                                             float* __restrict__ out_f) {
    out[0] = lambda_d * (s[0] / dl_at_least_one(s[1]));
    out[1] = lambda_tv * (s[2] / dl_at_least_one(s[3]) + s[4] / dl_at_least_one(s[5]));
    out[2] = s[1]; out[3] = s[3]; out[4] = s[5]; out[5] = s[2]; out[6] = s[4]; out[7] = (double)dmax;
    if (out_f != nullptr) {
        out_f[0] = (float)out[0]; out_f[1] = (float)out[1];
        out_f[2] = (float)((loss_base != nullptr ? (double)loss_base[0] : 0.0) + out[0] + out[1]);
    }
}

__global__ void __launch_bounds__(256)
depth_loss_finalize_kernel(int n_blocks, const double* __restrict__ partials, const float* __restrict__ max_slots,
                           double lambda_d, double lambda_tv, const float* __restrict__ loss_base,
                           double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kDlCols][4];
    __shared__ double s[kDlCols];
    dl_fold(n_blocks, partials, s_w, s);
    if (threadIdx.x == 0) dl_write_out(s, lambda_d, lambda_tv, n_blocks > 0 ? max_slots[kDlMaxSlot] : 0.f, loss_base,
                                           out, out_f);
}

// ---- the gradient pass -------------------------------------------------------------------------------------------------------
// RGB, NEIGHBOURS: as in the reduce pass; TV: the smoothness term is on (the left and upper neighbour are read too)
template <bool RGB, bool NEIGHBOURS, bool TV>
__global__ void __launch_bounds__(256)
depth_loss_grad_kernel(DlImage im, int n_blocks, const double* __restrict__ partials, const float* __restrict__ max_slots,
                       double lambda_d, double lambda_tv, const float* __restrict__ g_data, const float* __restrict__ g_tv,
                       const float* __restrict__ loss_base, float* __restrict__ v_depth, int v_depth_stride,
                       double* __restrict__ out, float* __restrict__ out_f) {
    __shared__ double s_w[kDlCols][4];
    __shared__ double s[kDlCols];
    dl_fold(n_blocks, partials, s_w, s);
    // the fully scaled weights, once per workgroup: upstream gradient * lambda / max(count, 1)
    const float wd = im.data ? (float)((g_data != nullptr ? (double)g_data[0] : 1.0) * lambda_d / dl_at_least_one(s[1])) : 0.f;
    const double gtv = im.tv ? (g_tv != nullptr ? (double)g_tv[0] : 1.0) * lambda_tv : 0.0;
    const float wx = (float)(gtv / dl_at_least_one(s[3])), wy = (float)(gtv / dl_at_least_one(s[5]));
    if (out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)     // (both passes in one call: no fold launch in between)
        dl_write_out(s, lambda_d, lambda_tv, max_slots[kDlMaxSlot], loss_base, out, out_f);

    // a workgroup walks 64 x 4 tiles (a wave per row piece): the upper and lower neighbours of the two inner rows are loads of
    // this workgroup; with 256 consecutive pixels of one row per workgroup every row was fetched three times
    const int W = im.W, tiles_x = (im.W + 63) / 64, n_tiles = tiles_x * ((im.H + kDlGradRows - 1) / kDlGradRows);
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x = tx * 64 + lx, y = ty * kDlGradRows + ly;
        if (x >= im.W || y >= im.H) continue;
        const size_t q = (size_t)y * W + x;
        const bool has_r = x < im.W - 1, has_l = x > 0, has_d = y < im.H - 1, has_u = y > 0;
        // every load of this pixel up front (a neighbour that does not exist: the pixel itself)
        const DlSite c = dl_load<RGB>(im, q);
        const DlSite r = NEIGHBOURS ? dl_load<RGB>(im, has_r ? q + 1 : q) : c;
        const DlSite dn = NEIGHBOURS ? dl_load<RGB>(im, has_d ? q + W : q) : c;
        const DlSite l = TV ? dl_load<RGB>(im, has_l ? q - 1 : q) : c;
        const DlSite up = TV ? dl_load<RGB>(im, has_u ? q - W : q) : c;
        const float gt = im.data ? im.gt[q] : 0.f;
        const float gx = RGB && has_r ? dl_cdiff(c, r) : 0.f, gy = RGB && has_d ? dl_cdiff(c, dn) : 0.f;
        // with the fix-up an alpha == 0 pixel holds the detached maximum: no gradient (and no pair) there
        const bool seen = !im.fixup || c.alpha > 0.f;
        float g = 0.f;
        if (im.data && seen) {
            float val, dval;
            if (dl_data(im, c.d, c.m, gt, gx, gy, &val, &dval)) g = wd * dval;
        }
        if (TV && dl_tv_ok(c)) {                              // (a fixed order: the sum's bits do not depend on the run)
            const bool e = im.tv_edge != 0;
            float t = 0.f;
            if (has_r && dl_tv_ok(r)) t -= wx * (e ? expf(-gx) : 1.f) * dl_sign(r.d - c.d);
            if (has_l && dl_tv_ok(l)) t += wx * (e ? expf(-dl_cdiff(l, c)) : 1.f) * dl_sign(c.d - l.d);
            if (has_d && dl_tv_ok(dn)) t -= wy * (e ? expf(-gy) : 1.f) * dl_sign(dn.d - c.d);
            if (has_u && dl_tv_ok(up)) t += wy * (e ? expf(-dl_cdiff(up, c)) : 1.f) * dl_sign(c.d - up.d);
            g += t;
        }
        v_depth[q * (size_t)v_depth_stride] = g;
    }
}

}  // namespace qed

using namespace qed;

extern "C" int qed_depth_loss(int32_t height, int32_t width, const float* depth, int32_t depth_stride, const float* alpha,
                              const float* dmax, const float* gt_depth, const float* mask, const float* gt_rgb, int32_t type,
                              float depth_lambda, float huber_delta, float tv_lambda, uint32_t flags, const float* g_data,
                              const float* g_tv, const float* loss_base, double* workspace, float* v_depth,
                              int32_t v_depth_stride, double* out, float* out_f, void* stream) {
    const int data = (flags & QED_DL_DATA) != 0, tv = (flags & QED_DL_TV) != 0, tv_edge = tv && (flags & QED_DL_TV_EDGE) != 0;
    const int fixup = (flags & QED_DL_FIXUP) != 0;
    const int reduce = (flags & QED_DL_REDUCE) != 0, grad = (flags & QED_DL_GRAD) != 0;
    QED_REQUIRE(height >= 0 && width >= 0, "negative size");
    QED_REQUIRE((flags & ~(uint32_t)(QED_DL_DATA | QED_DL_TV | QED_DL_TV_EDGE | QED_DL_FIXUP | QED_DL_REDUCE | QED_DL_GRAD)) == 0,
                "unknown flag");
    QED_REQUIRE(reduce || grad, "flags: QED_DL_REDUCE, QED_DL_GRAD or both");
    QED_REQUIRE(type >= QED_DL_L1 && type <= QED_DL_EDGE_LOGL1, "unknown depth loss type");
    QED_REQUIRE(!(data && type == QED_DL_HUBER) || (huber_delta > 0.f && huber_delta <= 3.4e38f), "huber_delta must be > 0");
    QED_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7) == 0, "workspace: doubles");
    QED_REQUIRE(!reduce || (out != nullptr && ((uintptr_t)out & 7) == 0), "out: 8 doubles");
    QED_REQUIRE(out == nullptr || ((uintptr_t)out & 7) == 0, "out: 8 doubles");
    const long long n_pix = (long long)height * width;
    QED_REQUIRE(n_pix <= 0x7fffffffLL, "image too large");
    if (n_pix > 0) {
        QED_REQUIRE(depth != nullptr && depth_stride >= 1, "null depth");
        QED_REQUIRE(!data || gt_depth != nullptr, "the data term needs the sensor depth");
        QED_REQUIRE(!(fixup || tv) || alpha != nullptr, "the fix-up and the smoothness term need alpha");
        QED_REQUIRE(!((data && type == QED_DL_EDGE_LOGL1) || tv_edge) || gt_rgb != nullptr,
                    "the edge-aware weights need the ground-truth colour");
        QED_REQUIRE(!grad || (v_depth != nullptr && v_depth_stride >= 1), "null output");
    }
    hipStream_t st = (hipStream_t)stream;
    DlImage im;
    im.H = height; im.W = width;
    im.depth = depth; im.depth_stride = depth_stride;
    im.alpha = alpha; im.gt = gt_depth; im.mask = mask; im.rgb = gt_rgb;
    im.type = type;
    im.delta = huber_delta; im.inv_delta = huber_delta > 0.f ? 1.f / huber_delta : 0.f;
    im.fixup = fixup; im.data = data; im.tv = tv; im.tv_edge = tv_edge;
    const bool rgb = (data && type == QED_DL_EDGE_LOGL1) || tv_edge;      // an edge-aware term reads the colour image
    const double lambda_d = data ? (double)depth_lambda : 0.0, lambda_tv = tv ? (double)tv_lambda : 0.0;
    float* max_slots = reinterpret_cast<float*>(workspace + (size_t)kDlCols * kDlMaxGrid);
    // (the grid is a function of the size alone: a gradient pass in a later call folds the same slots)
    const long long tiles_x = (width + 63) / 64;
    const unsigned grid = n_pix == 0 ? 0u : (unsigned)std::min<long long>(
        tiles_x * ((height + kDlReduceRows - 1) / kDlReduceRows), kDlMaxGrid);
    const unsigned grad_grid = (unsigned)std::min<long long>(tiles_x * ((height + kDlGradRows - 1) / kDlGradRows), 2048);
    if (reduce) {
        if (grid > 0) {
            const unsigned max_grid = stream_grid(n_pix, kDlMaxSlot);
            if (fixup && dmax == nullptr)
                hipLaunchKernelGGL(depth_loss_max_kernel, dim3(max_grid), dim3(256), 0, st, (int)n_pix, depth, depth_stride,
                                   max_slots);
            auto kernel = rgb ? depth_loss_reduce_kernel<true, true>
                              : (tv ? depth_loss_reduce_kernel<false, true> : depth_loss_reduce_kernel<false, false>);
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kDlReduceThreads), 0, st, im, dmax, (int)max_grid, max_slots,
                               workspace);
        }
        if (!grad || grid == 0)
            hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (int)grid, (const double*)workspace,
                               (const float*)max_slots, lambda_d, lambda_tv, loss_base, out, out_f);
    }
    if (grad && grid > 0) {
        auto kernel = rgb ? (tv ? depth_loss_grad_kernel<true, true, true> : depth_loss_grad_kernel<true, true, false>)
                          : (tv ? depth_loss_grad_kernel<false, true, true> : depth_loss_grad_kernel<false, false, false>);
        hipLaunchKernelGGL(kernel, dim3(grad_grid), dim3(256), 0, st, im, (int)grid,
                           (const double*)workspace, (const float*)max_slots, lambda_d, lambda_tv, g_data, g_tv, loss_base,
                           v_depth, v_depth_stride, reduce ? out : nullptr, reduce ? out_f : nullptr);
    }
    return check_launch("qed_depth_loss");
}
