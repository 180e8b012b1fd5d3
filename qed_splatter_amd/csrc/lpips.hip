// LPIPS (AlexNet) of two images from user-supplied weights: the `rgb_lpips` entry of get_metrics_dict (the reference's
// metrics.py:83-112 runs torchmetrics' LearnedPerceptualImagePatchSimilarity on every step and every eval image).
//
//   scaling   x' = (x - shift) / scale per channel, BEFORE conv1's zero padding (a padded tap contributes 0)
//   features  five convolution + bias + ReLU layers (table below), a 3x3 / stride 2 max-pool (no padding, floor) in front
//             of conv2 and of conv3
//   distance  per layer and pixel: unit-normalise both channel vectors, f / sqrt(eps + sum_c f^2) (eps INSIDE the root),
//             sum_c lin[c] (n0[c] - n1[c])^2; mean over the pixels; sum over the five layers
//
// Both images go through every launch as a batch of two.  Feature maps are NHWC ([2][Ho][Wo][C]): a row of the implicit
// GEMM (M = 2 Ho Wo, N = Cout, K = kh kw Cin with the channel fastest) then reads 16 consecutive channels of one filter
// tap per K tile, and the distance kernel reads a pixel's channel vector as one contiguous run.
//
// The convolution runs on the exact f32-input matrix instruction (v_mfma_f32_32x32x2_f32): its result is bit for bit a
// k-ordered fmaf chain, so every output element is the same chain of roundings wherever in a tile it sits -- the two
// images of a batch get identical bits from identical pixels (lpips(a, a) == 0 exactly) and a rerun repeats itself.
// No float atomics anywhere: per-workgroup partial sums, folded in a fixed order in float64 (as metrics.hip does).
#include "qed_common.h"

namespace qed {

constexpr float kLpipsEps = 1e-8f;                                     // inside the root of the channel norm
constexpr float kLpipsShift[3] = {-0.030f, -0.088f, -0.188f};         // the scaling layer in front of conv1
constexpr float kLpipsScale[3] = {0.458f, 0.448f, 0.450f};

constexpr int kLpipsLayers = 5;
constexpr int kLpipsCin[kLpipsLayers] = {3, 64, 192, 384, 256};
constexpr int kLpipsCout[kLpipsLayers] = {64, 192, 384, 256, 256};
constexpr int kLpipsKernel[kLpipsLayers] = {11, 5, 3, 3, 3};
constexpr int kLpipsStride[kLpipsLayers] = {4, 1, 1, 1, 1};
constexpr int kLpipsPad[kLpipsLayers] = {2, 2, 1, 1, 1};

// workgroup tile: 128 rows of M x 64 columns of N, K in steps of 16; four waves as 2 x 2, each 64 x 32 = two 32x32
// accumulators (two independent chains cover the instruction's 64-cycle dependent latency)
constexpr int kBM = 128, kBN = QED_LPIPS_TILE_N, kBK = QED_LPIPS_TILE_K;
// LDS row strides (words).  A: a store instruction's 32 lanes hold four k rows (q = 0..3, four rows apart) x eight
// consecutive m; 4 * 130 = 8 (mod 32) puts the four rows on banks 0, 8, 16, 24: conflict-free.  B: 68 * 4 B is a
// multiple of 16 (float4 stores)
constexpr int kLdA = kBM + 2, kLdB = kBN + 4;
constexpr int kDistMaxGrid = QED_LPIPS_WS_DOUBLES / kLpipsLayers;

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int conv_out(int in, int l) {
    const int span = in + 2 * kLpipsPad[l] - kLpipsKernel[l];
    return span < 0 ? 0 : span / kLpipsStride[l] + 1;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lpips_scale_tap(float x, int c) {
    const float sh = c == 0 ? kLpipsShift[0] : (c == 1 ? kLpipsShift[1] : kLpipsShift[2]);
    const float sc = c == 0 ? kLpipsScale[0] : (c == 1 ? kLpipsScale[1] : kLpipsScale[2]);
    return (x - sh) / sc;
}

// out[m][n] = relu(bias[n] + sum_k A[m][k] W[k][n]),  m = (image, oy, ox),  k = (kh, kw, c),  A gathered from the two
// NHWC inputs in0 / in1 ([Hi][Wi][CIN] each).  wp: [KP][NP] packed weights, zero beyond K and COUT (padded once at load
// time, so neither tail is tested in the loop).  Rows past M are loaded from row M - 1 and never stored.
// The order of the sum over k is k = 0, 1, 2, ... for every output element.
template <int CIN, int COUT, int KS, int STRIDE, int PAD, bool SCALE>
__global__ void __launch_bounds__(256)
lpips_conv_kernel(const float* __restrict__ in0, const float* __restrict__ in1, const float* __restrict__ wp,
                  const float* __restrict__ bias, float* __restrict__ out, int Hi, int Wi, int Ho, int Wo) {
    constexpr int K = CIN * KS * KS, KP = round_up(K, kBK), NP = round_up(COUT, kBN), NT = NP / kBN;
    constexpr bool kVec = CIN % kBK == 0;                  // a K tile is 16 consecutive channels of ONE tap
    __shared__ float As[kBK][kLdA];
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLdB];
    const int M = 2 * Ho * Wo;                             // (< 2^31: checked on the host)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
    const int n_blk = (int)(blockIdx.x % NT) * kBN;        // N tiles fastest: the workgroups that share an A tile run together
    const int m_blk = (int)(blockIdx.x / NT) * kBM;

    // the two rows of the A tile this thread gathers: row = t / 4 (+ 64), four consecutive k at q * 4
    const int q = t & 3;
    const float* base[2];
    int iy0[2], ix0[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = min(m_blk + (t >> 2) + 64 * r, M - 1);
        const int img = m / (Ho * Wo), rem = m - img * (Ho * Wo);      // a row never mixes the two images
        const int oy = rem / Wo, ox = rem - oy * Wo;
        base[r] = img ? in1 : in0;
        iy0[r] = oy * STRIDE - PAD;
        ix0[r] = ox * STRIDE - PAD;
    }
    auto load_a = [&](int k0, float (&v)[2][4]) {
        if constexpr (kVec) {
            const int tap = k0 / CIN, c = k0 - tap * CIN + q * 4, kh = tap / KS, kw = tap - kh * KS;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int iy = iy0[r] + kh, ix = ix0[r] + kw;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
                    x = *reinterpret_cast<const float4*>(base[r] + ((size_t)iy * Wi + ix) * CIN + c);
                v[r][0] = x.x; v[r][1] = x.y; v[r][2] = x.z; v[r][3] = x.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + q * 4 + j, tap = k / CIN, c = k - tap * CIN, kh = tap / KS, kw = tap - kh * KS;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int iy = iy0[r] + kh, ix = ix0[r] + kw;
                    float x = 0.f;                         // padding and the K tail: exactly 0, after the scaling
                    if (k < K && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) {
                        x = base[r][((size_t)iy * Wi + ix) * CIN + c];
                        if constexpr (SCALE) x = lpips_scale_tap(x, c);
                    }
                    v[r][j] = x;
                }
            }
        }
    };
    // B tile: 16 x 64 floats = one float4 per thread
    const int bk = t >> 4, bn = (t & 15) * 4;
    auto load_b = [&](int k0) { return *reinterpret_cast<const float4*>(wp + (size_t)(k0 + bk) * NP + n_blk + bn); };

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    float ra[2][4];
    float4 rb;
    load_a(0, ra);
    rb = load_b(0);
    for (int k0 = 0; k0 < KP; k0 += kBK) {
        __syncthreads();                                   // the previous tile has been read
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) As[q * 4 + j][(t >> 2) + 64 * r] = ra[r][j];
        *reinterpret_cast<float4*>(&Bs[bk][bn]) = rb;
        __syncthreads();
        if (k0 + kBK < KP) {                               // the next tile's loads fly while this one is multiplied
            load_a(k0 + kBK, ra);
            rb = load_b(k0 + kBK);
        }
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 2) {
            // operand maps of 32x32x2: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
            const int kr = kk + (lane >> 5);
            const float b = Bs[kr][wn * 32 + (lane & 31)];
            const float a0 = As[kr][wm * 64 + (lane & 31)];
            const float a1 = As[kr][wm * 64 + 32 + (lane & 31)];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
        }
    }
    // C/D map of 32x32: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The M tail is tested here only.
    const int n = n_blk + wn * 32 + (lane & 31);
    if (n >= COUT) return;
    const float bv = bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m_blk + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (m < M) out[(size_t)m * COUT + n] = fmaxf(acc[i][e] + bv, 0.f);
        }
}

// 3x3 max-pool, stride 2, no padding, floor: in [2][Hi][Wi][C] -> out [2][Ho][Wo][C], four channels per thread.  Every
// window lies inside its own image (2 (Ho - 1) + 2 <= Hi - 1), so none crosses the batch seam.
__global__ void __launch_bounds__(256)
lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int C4, int Hi, int Wi, int Ho, int Wo) {
    const size_t total = (size_t)2 * Ho * Wo * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        size_t p = i / C4;
        const int ox = (int)(p % Wo);
        p /= Wo;
        const int oy = (int)(p % Ho), img = (int)(p / Ho);
        const float4* src = reinterpret_cast<const float4*>(in) + (((size_t)img * Hi + 2 * oy) * Wi + 2 * ox) * C4 + c4;
        float4 m = src[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const float4 v = src[((size_t)dy * Wi + dx) * C4];
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        reinterpret_cast<float4*>(out)[i] = m;
    }
}

// One wave per pixel, CPL = C / 64 channels per lane held in registers between the norm and the difference.
// partials[block]: the workgroup's sum over its pixels of sum_c lin[c] (f0[c] / |f0| - f1[c] / |f1|)^2.
template <int CPL>
__global__ void __launch_bounds__(256)
lpips_distance_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int n_pix, double* __restrict__ partials) {
    // no contraction here: a / na - b / nb fused into fma(b, 1 / nb, -(rounded a / na)) leaves the rounding error of the
    // first quotient behind, and identical images would not give exactly 0
#pragma clang fp contract(off)
    constexpr int C = CPL * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* f0 = feat;
    const float* f1 = feat + (size_t)n_pix * C;
    float w[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) w[j] = lin[j * 64 + lane];
    float acc = 0.f;
    for (int p = blockIdx.x * 4 + wave; p < n_pix; p += gridDim.x * 4) {
        float a[CPL], b[CPL], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            a[j] = f0[(size_t)p * C + j * 64 + lane];
            b[j] = f1[(size_t)p * C + j * 64 + lane];
            sa += a[j] * a[j];
            sb += b[j] * b[j];
        }
        const float na = sqrtf(kLpipsEps + wave_sum(sa)), nb = sqrtf(kLpipsEps + wave_sum(sb));
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float e = a[j] / na - b[j] / nb;
            d += w[j] * (e * e);
        }
        acc += wave_sum(d);
    }
    const double v[1] = {(double)acc};                        // already a wave's sum, the same in every lane
    __shared__ double s_w[1][4];
    __shared__ double s[1];
    block_combine_d(v, s_w, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

struct LpipsFold {
    int n_blocks[kLpipsLayers];
    long long n_pix[kLpipsLayers];
};

// out[1 + l] = mean over the pixels of layer l's distance, out[0] = their sum; one workgroup, float64, fixed order
__global__ void __launch_bounds__(256)
lpips_finalize_kernel(LpipsFold f, const double* __restrict__ partials, float* __restrict__ out) {
    static_assert(kDistMaxGrid == 256, "one partial per thread");
    __shared__ double s_w[kLpipsLayers][4];
    __shared__ double s[kLpipsLayers];
    double v[kLpipsLayers];
#pragma unroll
    for (int l = 0; l < kLpipsLayers; ++l)
        v[l] = (int)threadIdx.x < f.n_blocks[l] ? partials[l * kDistMaxGrid + threadIdx.x] : 0.0;
    block_sum_d(v, s_w, s);
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int l = 0; l < kLpipsLayers; ++l) {
        const double term = s[l] / (double)f.n_pix[l];
        out[1 + l] = (float)term;
        total += term;
    }
    out[0] = (float)total;
}

inline int dist_grid(long long n_pix) {
    long long g = (n_pix + 3) / 4;
    return (int)(g > kDistMaxGrid ? kDistMaxGrid : g);
}

template <int L>
static void launch_conv(const float* in0, const float* in1, const float* wp, const float* bias, float* out, int Hi, int Wi,
                        int Ho, int Wo, hipStream_t st) {
    constexpr int NT = round_up(kLpipsCout[L], kBN) / kBN;
    const long long m_tiles = (2LL * Ho * Wo + kBM - 1) / kBM;
    hipLaunchKernelGGL((lpips_conv_kernel<kLpipsCin[L], kLpipsCout[L], kLpipsKernel[L], kLpipsStride[L], kLpipsPad[L], L == 0>),
                       dim3((unsigned)(m_tiles * NT)), dim3(256), 0, st, in0, in1, wp, bias, out, Hi, Wi, Ho, Wo);
}

}  // namespace qed

using namespace qed;

extern "C" int64_t qed_lpips_packed_floats(int32_t layer) {
    if (layer < 0 || layer >= kLpipsLayers) {
        set_error("qed_lpips_packed_floats: layer must be 0..4");
        return QED_E_INVALID_ARG;
    }
    const int K = kLpipsCin[layer] * kLpipsKernel[layer] * kLpipsKernel[layer];
    return (int64_t)round_up(K, kBK) * round_up(kLpipsCout[layer], kBN);
}

extern "C" int qed_lpips_conv(int32_t layer, int32_t in_h, int32_t in_w, const float* in0, const float* in1,
                              const float* weights, const float* bias, float* out, void* stream) {
    QED_REQUIRE(layer >= 0 && layer < kLpipsLayers, "layer must be 0..4");
    QED_REQUIRE(in_h >= 1 && in_w >= 1 && in_h <= 32768 && in_w <= 32768, "input size out of range");
    QED_REQUIRE(in0 && in1 && weights && bias && out, "null buffer");
    const int Ho = conv_out(in_h, layer), Wo = conv_out(in_w, layer);
    QED_REQUIRE(Ho >= 1 && Wo >= 1, "input smaller than the filter");
    QED_REQUIRE(2LL * Ho * Wo < (1LL << 30), "too many output pixels");
    hipStream_t st = (hipStream_t)stream;
    switch (layer) {
        case 0: launch_conv<0>(in0, in1, weights, bias, out, in_h, in_w, Ho, Wo, st); break;
        case 1: launch_conv<1>(in0, in1, weights, bias, out, in_h, in_w, Ho, Wo, st); break;
        case 2: launch_conv<2>(in0, in1, weights, bias, out, in_h, in_w, Ho, Wo, st); break;
        case 3: launch_conv<3>(in0, in1, weights, bias, out, in_h, in_w, Ho, Wo, st); break;
        default: launch_conv<4>(in0, in1, weights, bias, out, in_h, in_w, Ho, Wo, st); break;
    }
    return check_launch("qed_lpips_conv");
}

extern "C" int qed_lpips_pool(int32_t channels, int32_t in_h, int32_t in_w, const float* in, float* out, void* stream) {
    QED_REQUIRE(channels >= 4 && channels % 4 == 0 && channels <= 4096, "channels must be a multiple of 4");
    QED_REQUIRE(in_h >= 3 && in_w >= 3 && in_h <= 32768 && in_w <= 32768, "input smaller than the 3x3 window");
    QED_REQUIRE(in && out, "null buffer");
    const int Ho = (in_h - 3) / 2 + 1, Wo = (in_w - 3) / 2 + 1;
    const long long total = 2LL * Ho * Wo * (channels / 4);
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(stream_grid(total, 8192)), dim3(256), 0, (hipStream_t)stream, in, out,
                       channels / 4, in_h, in_w, Ho, Wo);
    return check_launch("qed_lpips_pool");
}

extern "C" int qed_lpips_distance(int32_t layer, int32_t height, int32_t width, const float* feat, const float* lin,
                                  double* workspace, void* stream) {
    QED_REQUIRE(layer >= 0 && layer < kLpipsLayers, "layer must be 0..4");
    QED_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1LL << 29), "feature map size out of range");
    QED_REQUIRE(feat && lin && workspace, "null buffer");
    const int n_pix = height * width, g = dist_grid(n_pix);
    double* part = workspace + layer * kDistMaxGrid;
    hipStream_t st = (hipStream_t)stream;
    switch (kLpipsCout[layer] / 64) {
        case 1: hipLaunchKernelGGL(lpips_distance_kernel<1>, dim3(g), dim3(256), 0, st, feat, lin, n_pix, part); break;
        case 3: hipLaunchKernelGGL(lpips_distance_kernel<3>, dim3(g), dim3(256), 0, st, feat, lin, n_pix, part); break;
        case 6: hipLaunchKernelGGL(lpips_distance_kernel<6>, dim3(g), dim3(256), 0, st, feat, lin, n_pix, part); break;
        default: hipLaunchKernelGGL(lpips_distance_kernel<4>, dim3(g), dim3(256), 0, st, feat, lin, n_pix, part); break;
    }
    return check_launch("qed_lpips_distance");
}

extern "C" int qed_lpips_finalize(int64_t n_pix0, int64_t n_pix1, int64_t n_pix2, int64_t n_pix3, int64_t n_pix4,
                                  const double* workspace, float* out, void* stream) {
    const int64_t n[kLpipsLayers] = {n_pix0, n_pix1, n_pix2, n_pix3, n_pix4};
    LpipsFold f;
    for (int l = 0; l < kLpipsLayers; ++l) {
        QED_REQUIRE(n[l] >= 1 && n[l] < (1LL << 29), "pixel counts out of range");
        f.n_pix[l] = n[l];
        f.n_blocks[l] = dist_grid(n[l]);
    }
    QED_REQUIRE(workspace && out, "null buffer");
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, f, workspace, out);
    return check_launch("qed_lpips_finalize");
}
