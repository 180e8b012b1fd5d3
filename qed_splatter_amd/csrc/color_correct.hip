// Colour correction of an evaluation render against its ground truth (qed_color_correct): nerfstudio's
// lib_bilagrid.color_correct, a port of multinerf's, behind SplatfactoModelConfig.color_corrected_metrics.
//
//   x = img, r = ref ([n_pix,3] in [0,1]); unclipped(z) = (z >= eps) & (z <= 1 - eps); mask0 = unclipped(img), once.
//   num_iters times:  a(x) = (rr, rg, rb, gg, gb, bb, r, g, b, 1)  -- x[c] * x[c:] for c = 0, 1, 2, the linear terms, 1;
//                     m_c  = mask0[c] & unclipped(x[c]) & unclipped(r[c]);
//                     w_c  = least-squares solution of (m_c a) w = m_c r[c];     x <- clip(a(x) [w_0 w_1 w_2], 0, 1)
//
// Upstream solves the 15 systems with torch.linalg.lstsq on a [n_pix, 10] matrix.  Here every system is its normal
// equations: Sum m_c a a^T (55 distinct entries) and Sum m_c a r[c] (10), three channels = 195 sums per iteration, carried
// in DOUBLE (a product of two float32 features is exact in double; a float32 Gram matrix loses cond(A)^2 * 6e-8), and a
// 10 x 10 solve in double on the device.  No intermediate image exists: iteration k's pixels are rebuilt in registers from
// the original pixel and the k earlier warps, in float32 (cc_current: ONE function, used by both passes, explicit fmas,
// so that every launch sees the same bits).  Per iteration the image and the ground truth are read once, 24 B per pixel.
//
// How the 195 sums are held.  KEPT: the f64 matrix instruction.  With A = [m_0 a; m_1 a; m_2 a] (30 rows, padded to 32)
// and B = [a | r_0 r_1 r_2 | m_0 m_1 m_2] (16 columns), A B^T over the pixels holds every sum needed (the full 10 x 10
// blocks; only the lower triangles and column 10 + c of block c are stored).  v_mfma_f64_16x16x4_f64 takes four pixels
// per issue: lane l supplies A[row l & 15][pixel l >> 4] and B[pixel l >> 4][column l & 15], and holds
// D[row (l >> 4) + 4 reg][column l & 15], reg 0..3.  A wave stages its 64 pixels' 16 doubles each in a private 8 KB
// of LDS (features as exact double products), then sixteen steps of five LDS reads, two multiplies by the mask and two
// matrix instructions (rows 0-15 and 16-31) consume them; a lane's accumulators are 8 doubles.  The sums of a wave are
// deterministic; waves park theirs in LDS and are added in the fixed order of combine_waves; every workgroup writes its
// 195 sums to its own slots and the one-workgroup solve launch folds them in a fixed order (qed_reduce.h's pattern, no
// floating-point atomics): two runs give the same bits.
// 512 threads per workgroup under at most 512 workgroups: twice the resident waves of a 256-thread build for the same
// number of partial-sum slots.  The pass is bound by the matrix pipe and the staging, not by memory: 2.1 GFLOP per
// iteration are 27 us at the f64 matrix peak.
// THE OTHER CANDIDATE was the same LDS staging with one owned sum per thread (195 of 256 threads, every thread walks all
// rows of the chunk: three LDS reads and two double multiply-adds per pixel and thread).  Built as a measurement variant,
// checked against the same parity tests, measured and then taken out again.  At 1920 x 1080 on one box, 100 launches
// each, average per launch (profiles/color_correct.txt): matrix instruction, 512 threads 70.5 us (KEPT); matrix
// instruction, 256 threads 76.4 us; one owned sum per thread 205.8 us.
// A wave consumes only the rows it staged itself, so inside the loop its LDS writes and reads are ordered at wave level
// (cc_wave_sync); the one workgroup barrier stands before the parking.  With barriers in the loop, as in the A/B above,
// the pass took 70.5 us; as it stands 66.3 us.
// Registers / scratch (scripts/kernel_resources.sh, gfx950): summing pass 82 VGPRs, 64 KB LDS, no scratch, 4 waves per
// SIMD; solve 63 VGPRs; last pass 17 VGPRs, no scratch in any (profiles/color_correct.txt).
//
// The solver: Cholesky with diagonal pivoting in double.  A column whose remaining pivot is <= 1e-10 x the largest
// ORIGINAL diagonal entry is dropped and its coefficient is 0 -- a stated deviation: upstream's lstsq returns the
// minimum-norm solution; both have the same fitted values on the pixels of the fit.  A channel without an unmasked pixel
// gets w = 0 and comes out 0, as upstream's does.  A pixel with a non-finite value in img or ref takes part in no fit
// (whatever eps is; so does no lane past n_pix); where it is warped, its non-finite values are read as 0.  With
// num_iters >= 1 no input produces a NaN: the clip maps NaN to 0, a non-finite coefficient is replaced by 0.  With
// num_iters == 0 out is img itself, bit for bit, non-finite values included.
#include "qed_common.h"

namespace qed {

constexpr int kCcFeat = 10;
constexpr int kCcChanSums = 65;                               // 55 of the lower triangle of Sum m a a^T, 10 of Sum m a r
constexpr int kCcSums = 3 * kCcChanSums;                      // 195
constexpr int kCcStride = QED_COLOR_CORRECT_SUMS_STRIDE;      // doubles per workgroup in the workspace
constexpr int kCcMaxGrid = QED_COLOR_CORRECT_MAX_GRID;
constexpr int kCcWarpFloats = 3 * kCcFeat;                    // one iteration's warp, [channel][feature], float32
static_assert(kCcStride >= kCcSums, "a workgroup's slots hold its sums");
static_assert(QED_COLOR_CORRECT_WS_DOUBLES >= kCcMaxGrid * kCcStride + (QED_COLOR_CORRECT_MAX_ITERS * kCcWarpFloats + 1) / 2,
              "workspace: the partial sums, then the float32 warps");

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float cc_finite_or_zero(float v) { return isfinite(v) ? v : 0.f; }

__device__ __forceinline__ bool cc_unclipped(float v, float lo, float hi) { return v >= lo && v <= hi; }

// x <- clip(a(x) W, 0, 1) in float32; W: [3][10].  The order of the fmas is part of the definition (see the header).
__device__ __forceinline__ void cc_apply_warp(float (&x)[3], const float* __restrict__ W) {
    const float a[9] = {__fmul_rn(x[0], x[0]), __fmul_rn(x[0], x[1]), __fmul_rn(x[0], x[2]), __fmul_rn(x[1], x[1]),
                        __fmul_rn(x[1], x[2]), __fmul_rn(x[2], x[2]), x[0], x[1], x[2]};
    float y[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = W[c * kCcFeat + 9];
#pragma unroll
        for (int f = 8; f >= 0; --f) acc = __fmaf_rn(a[f], W[c * kCcFeat + f], acc);
        y[c] = fminf(fmaxf(acc, 0.f), 1.f);                   // (fmaxf returns the other operand for NaN: NaN -> 0)
    }
    x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
}

// the pixel after the first n_warps iterations
__device__ __forceinline__ void cc_current(float (&x)[3], int n_warps, const float* __restrict__ warps) {
    for (int k = 0; k < n_warps; ++k) cc_apply_warp(x, warps + k * kCcWarpFloats);
}

// ---- pass 1 of an iteration: the 195 sums of every workgroup -----------------------------------------------------------
// LDS row of a pixel, 16 doubles: 0-9 a(x), 10-12 r, 13-15 m_0 m_1 m_2 (0.0 / 1.0).
constexpr int kCcThreads = 512;                               // threads of the summing pass
constexpr int kCcWaves = kCcThreads / 64;

// A wave reads only the rows it staged itself: between its LDS writes and reads (and back) it needs no workgroup barrier,
// only that the compiler keeps the order; LDS operations of one wave complete in the order they were issued.
__device__ __forceinline__ void cc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(kCcThreads)
cc_accumulate_kernel(int n_pix, const float* __restrict__ img, const float* __restrict__ ref, int n_warps,
                     const float* __restrict__ warps, float lo, float hi, double* __restrict__ partials) {
    __shared__ double s_mem[kCcThreads * 16];                 // a row per thread's pixel; afterwards the parked sums
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double* stage = s_mem + wid * (64 * 16);                  // this wave's 64 rows
    // rows of A this lane supplies: R0 = l & 15 (tile 0), R1 = 16 + (l & 15) (tile 1; 30 and 31 are padding whose
    // results are not stored); row R = 10 c + f is feature f under channel c's mask
    const int rowl = lane & 15, kq = lane >> 4;
    const int c0 = rowl / kCcFeat, f0 = rowl % kCcFeat;
    const int R1 = 16 + rowl;
    const int c1 = R1 < 30 ? R1 / kCcFeat : 0, f1 = R1 < 30 ? R1 % kCcFeat : 0;
    const double* pA0 = stage + kq * 16 + f0;
    const double* pM0 = stage + kq * 16 + 13 + c0;
    const double* pA1 = stage + kq * 16 + f1;
    const double* pM1 = stage + kq * 16 + 13 + c1;
    const double* pB = stage + kq * 16 + rowl;
    v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};

    const size_t stride = (size_t)gridDim.x * kCcThreads;
    // -> does the pixel exist?  (a lane past the end reads nothing and is excluded by its index, whatever eps is)
    auto load = [&](size_t base, float (&x)[3], float (&r)[3]) {
        const size_t i = base + tid;
        const bool in = i < (size_t)n_pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = in ? img[3 * i + c] : 0.f;
            r[c] = in ? ref[3 * i + c] : 0.f;
        }
        return in;
    };
    float nx[3], nr[3];
    bool n_in = load((size_t)blockIdx.x * kCcThreads, nx, nr);
    // (the trip count is the same for every wave of the workgroup; only the barrier behind the loop relies on all arriving)
    for (size_t base = (size_t)blockIdx.x * kCcThreads; base < (size_t)n_pix; base += stride) {
        float x[3], r[3];
        bool m[3];
        // a pixel takes part in the fits if it exists and all six of its values are finite -- decided on the index and
        // the raw values, never on what they are read as (with eps = 0 a 0 is unclipped)
        bool valid = n_in;
#pragma unroll
        for (int c = 0; c < 3; ++c) valid = valid && isfinite(nx[c]) && isfinite(nr[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = cc_finite_or_zero(nx[c]);
            r[c] = cc_finite_or_zero(nr[c]);
            m[c] = valid && cc_unclipped(x[c], lo, hi) && cc_unclipped(r[c], lo, hi);    // mask0 and the ground truth's
        }
        if (base + stride < (size_t)n_pix) n_in = load(base + stride, nx, nr);       // the next trip's loads, in flight
        cc_current(x, n_warps, warps);
        const double d0 = (double)x[0], d1 = (double)x[1], d2 = (double)x[2];
        double row[16] = {d0 * d0, d0 * d1, d0 * d2, d1 * d1, d1 * d2, d2 * d2, d0, d1, d2, 1.0,
                          (double)r[0], (double)r[1], (double)r[2], 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) row[13 + c] = (m[c] && cc_unclipped(x[c], lo, hi)) ? 1.0 : 0.0;
        double2* dst = reinterpret_cast<double2*>(stage + lane * 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = make_double2(row[2 * j], row[2 * j + 1]);
        cc_wave_sync();
#pragma unroll
        for (int s = 0; s < 16; ++s) {                        // pixels 4 s .. 4 s + 3 of the wave's 64
            const int o = s * 64;
            const double b = pB[o];
            const double a0 = pA0[o] * pM0[o];
            const double a1 = pA1[o] * pM1[o];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1, 0, 0, 0);
        }
        cc_wave_sync();
    }
    __syncthreads();                                          // every wave is done with its rows: the parking reuses them
    // park the waves' sums: s_mem[wave][j = tile * 4 + reg][lane]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        s_mem[(wid * 8 + g) * 64 + lane] = acc0[g];
        s_mem[(wid * 8 + 4 + g) * 64 + lane] = acc1[g];
    }
    __syncthreads();
    double* mine = partials + (size_t)blockIdx.x * kCcStride;
    for (int idx = tid; idx < 8 * 64; idx += kCcThreads) {
        const int j = idx >> 6, l = idx & 63;
        double w[kCcWaves];
#pragma unroll
        for (int k = 0; k < kCcWaves; ++k) w[k] = s_mem[(k * 8 + j) * 64 + l];
        const double v = combine_waves<kCcWaves>(w);
        const int R = 16 * (j >> 2) + (l >> 4) + 4 * (j & 3), col = l & 15;      // D[row (l >> 4) + 4 reg][col l & 15]
        if (R >= 30) continue;
        const int c = R / kCcFeat, f = R % kCcFeat;
        if (col <= f) mine[c * kCcChanSums + f * (f + 1) / 2 + col] = v;
        else if (col == kCcFeat + c) mine[c * kCcChanSums + 55 + f] = v;
    }
}

// ---- the 10 x 10 solve: Cholesky with diagonal pivoting, double, one thread per channel, everything in LDS -------------
__device__ void cc_solve(const double (*G)[kCcFeat], const double* b, double (*Lm)[kCcFeat], double* d, int* perm,
                         double* w) {
    double dmax = 0.0;
    for (int i = 0; i < kCcFeat; ++i) {
        d[i] = G[i][i];
        perm[i] = i;
        w[i] = 0.0;
        dmax = fmax(dmax, d[i]);
    }
    const double tol = 1e-10 * dmax;
    int rank = 0;
    for (int k = 0; k < kCcFeat; ++k) {
        int p = k;
        double best = d[k];
        for (int i = k + 1; i < kCcFeat; ++i)
            if (d[i] > best) { best = d[i]; p = i; }
        if (!(best > tol)) break;                             // this column and every remaining one is dropped
        if (p != k) {
            const int tp = perm[k]; perm[k] = perm[p]; perm[p] = tp;
            const double td = d[k]; d[k] = d[p]; d[p] = td;
            for (int j = 0; j < k; ++j) { const double t = Lm[k][j]; Lm[k][j] = Lm[p][j]; Lm[p][j] = t; }
        }
        const double lkk = sqrt(best);
        Lm[k][k] = lkk;
        for (int i = k + 1; i < kCcFeat; ++i) {
            double v = G[perm[i]][perm[k]];
            for (int j = 0; j < k; ++j) v -= Lm[i][j] * Lm[k][j];
            v /= lkk;
            Lm[i][k] = v;
            d[i] -= v * v;
        }
        rank = k + 1;
    }
    for (int i = 0; i < rank; ++i) {                          // L y = P b   (y in d)
        double v = b[perm[i]];
        for (int j = 0; j < i; ++j) v -= Lm[i][j] * d[j];
        d[i] = v / Lm[i][i];
    }
    for (int i = rank - 1; i >= 0; --i) {                     // L^T z = y   (z in d)
        double v = d[i];
        for (int j = i + 1; j < rank; ++j) v -= Lm[j][i] * d[j];
        d[i] = v / Lm[i][i];
        w[perm[i]] = isfinite(d[i]) ? d[i] : 0.0;
    }
}

// ---- pass 2 of an iteration: fold the workgroups' sums in a fixed order, solve, write the warp --------------------------
__global__ void __launch_bounds__(1024)
cc_solve_kernel(int n_blocks, const double* __restrict__ partials, float* __restrict__ warp_f, double* __restrict__ warp_d) {
    __shared__ double s_q[4][256];
    __shared__ double s_G[3][kCcFeat][kCcFeat], s_L[3][kCcFeat][kCcFeat], s_b[3][kCcFeat], s_d[3][kCcFeat], s_w[3][kCcFeat];
    __shared__ int s_perm[3][kCcFeat];
    const int tid = threadIdx.x, e = tid & 255, q = tid >> 8;
    // quarter q of the workgroups, in index order; the four quarters as (q0 + q1) + (q2 + q3)
    const int per = (n_blocks + 3) / 4;
    const int b0 = min(q * per, n_blocks), b1 = min(b0 + per, n_blocks);
    double sum = 0.0;
    if (e < kCcSums) {
        int b = b0;
        for (; b + 16 <= b1; b += 16) {                       // sixteen loads in flight, added in index order
            double t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = partials[(size_t)(b + u) * kCcStride + e];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += t[u];
        }
        for (; b < b1; ++b) sum += partials[(size_t)b * kCcStride + e];
    }
    s_q[q][e] = sum;
    __syncthreads();
    if (tid < kCcSums) {
        const double w[4] = {s_q[0][tid], s_q[1][tid], s_q[2][tid], s_q[3][tid]};
        const double tot = combine_waves<4>(w);
        const int c = tid / kCcChanSums, k = tid % kCcChanSums;
        if (k < 55) {
            int f = 0;
            while ((f + 1) * (f + 2) / 2 <= k) ++f;
            const int col = k - f * (f + 1) / 2;
            s_G[c][f][col] = tot;
            s_G[c][col][f] = tot;
        } else {
            s_b[c][k - 55] = tot;
        }
    }
    __syncthreads();
    if ((tid & 63) == 0 && (tid >> 6) < 3) {
        const int c = tid >> 6;
        cc_solve(s_G[c], s_b[c], s_L[c], s_d[c], s_perm[c], s_w[c]);
    }
    __syncthreads();
    if (tid < kCcWarpFloats) {
        const double v = s_w[tid / kCcFeat][tid % kCcFeat];
        warp_f[tid] = (float)v;
        if (warp_d != nullptr) warp_d[tid] = v;
    }
}

// ---- the last pass: clip(a W, 0, 1) of the final iteration --------------------------------------------------------------
__global__ void __launch_bounds__(256)
cc_apply_kernel(int n_pix, const float* __restrict__ img, int n_warps, const float* __restrict__ warps,
                float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n_pix; i += (size_t)gridDim.x * 256) {
        float x[3] = {img[3 * i], img[3 * i + 1], img[3 * i + 2]};
        if (n_warps > 0) {                                    // (no iteration: the input as it is)
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = cc_finite_or_zero(x[c]);
            cc_current(x, n_warps, warps);
        }
        out[3 * i] = x[0]; out[3 * i + 1] = x[1]; out[3 * i + 2] = x[2];
    }
}

}  // namespace qed

using namespace qed;

extern "C" int qed_color_correct(int32_t n_pix, const float* img, const float* ref, int32_t num_iters, float eps,
                                 double* workspace, double* warps_out, float* out, void* stream) {
    QED_REQUIRE(n_pix >= 0 && num_iters >= 0 && num_iters <= QED_COLOR_CORRECT_MAX_ITERS, "bad sizes (num_iters: 0 to 8)");
    QED_REQUIRE(eps >= 0.f && eps < 0.5f, "eps must lie in [0, 0.5)");
    if (n_pix == 0) return QED_OK;
    QED_REQUIRE(img && ref && out && workspace, "null pointer");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)warps_out & 7) == 0, "misaligned double pointer");
    hipStream_t st = (hipStream_t)stream;
    long long g = ((long long)n_pix + kCcThreads - 1) / kCcThreads;
    if (g > kCcMaxGrid) g = kCcMaxGrid;
    float* warps = reinterpret_cast<float*>(workspace + (size_t)kCcMaxGrid * kCcStride);
    const float lo = eps, hi = 1.0f - eps;
    for (int it = 0; it < num_iters; ++it) {
        hipLaunchKernelGGL(cc_accumulate_kernel, dim3((unsigned)g), dim3(kCcThreads), 0, st, n_pix, img, ref, it,
                           (const float*)warps, lo, hi, workspace);
        hipLaunchKernelGGL(cc_solve_kernel, dim3(1), dim3(1024), 0, st, (int)g, (const double*)workspace,
                           warps + it * kCcWarpFloats, warps_out != nullptr ? warps_out + it * kCcWarpFloats : nullptr);
    }
    hipLaunchKernelGGL(cc_apply_kernel, dim3(stream_grid(n_pix)), dim3(256), 0, st, n_pix, img, num_iters,
                       (const float*)warps, out);
    return check_launch("qed_color_correct");
}
