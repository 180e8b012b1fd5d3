// Splatfacto's strategy="mcmc" (gsplat MCMCStrategy): a fixed Gaussian budget, relocation of dead Gaussians, position
// noise every step and two regularisers, on the flat parameter / Adam-moment buffers of this package (group order
// means, scales, quats, opacities, features_dc, features_rest; the layout densify.hip writes).
//
//   weights / scan / prefix   sampling weights as integers (sigma 2^32 rounded, >= 1 for a live row, 0 otherwise) and
//                             their exact inclusive prefix (uint64): a draw is a binary search for an integer uniform
//   draw                      relocate: one source per dead slot; add / sample: n draws; ratio counts by int atomics
//   update                    opacity 1 - (1 - sigma)^(1/ratio) and the scale factor of every drawn source, in fp64
//   copy / emit               dead slots <- their source (in place) | old rows + appended copies (new buffers)
//   noise                     means += Sigma (eps gate lr noise_lr), eps from a counter-based generator
//   reg                       lambda_o mean(sigma), lambda_s mean(exp(log_scale)) + their gradients (fixed-order fold)
//
// Every random number is a function of (seed, counter or step, row index): equal seeds give bit-identical results on
// every data-parallel replica and in every replay of a captured graph.  The relocation never reads a row that the same
// launch rewrites: sources are updated in one launch and copied in the next.
#include <algorithm>

#include "qed_common.h"

namespace qed {

constexpr int kMcmcNMax = 51;                 // gsplat's n_max: the ratio is clamped to [1, 51]
constexpr int kMcmcRegBlocks = 1024;          // reg pass grid (block partials: 2 doubles each)
static_assert(2 * kMcmcRegBlocks <= QED_MCMC_REG_WS_DOUBLES, "reg workspace");

// (the counter-based generator mix64 / rng64 and its stream numbers: qed_common.h)

// sampling weight of a row: sigma 2^32 rounded, at least 1, for sigma > thresh; 0 otherwise (NaN included)
__device__ __forceinline__ unsigned long long draw_weight(float logit, float thresh) {
    const float s = sigmoidf_dev(logit);
    if (!(s > thresh)) return 0ull;
    const unsigned long long w = (unsigned long long)llrint((double)s * 4294967296.0);
    return w > 0ull ? w : 1ull;
}

__device__ __forceinline__ bool is_dead(float logit, float min_opacity) { return !(sigmoidf_dev(logit) > min_opacity); }

// first row whose inclusive prefix exceeds u (u < cdf[N-1]): never a zero-weight row
__device__ __forceinline__ int search_cdf(const unsigned long long* __restrict__ cdf, int N, unsigned long long u) {
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ int draw_row(const unsigned long long* __restrict__ cdf, int N, unsigned long long total,
                                        unsigned long long h) {
    return search_cdf(cdf, N, __umul64hi(h, total));                               // uniform on [0, total)
}

// ---- the exact integer prefix of the weights (3 launches) ----------------------------------------------------------
struct McmcWs {
    unsigned long long* cdf;      // [N]   inclusive prefix of the weights
    unsigned long long* block;    // [nb]  per-workgroup weight sums -> exclusive bases
    int* block_dead;              // [nb]  per-workgroup dead counts
    unsigned long long* total;    // [1]   sum of the weights
    int* counts;                  // [N]   times each row was drawn
    int* src;                     // [max(N, n_draws)] drawn source per slot / per draw
};

inline long long align256(long long b) { return (b + 255) & ~255ll; }

inline long long ws_bytes(long long N, long long n_draws) {
    const long long nb = (N + 255) / 256;
    return align256(8 * N) + align256(8 * nb) + align256(4 * nb) + align256(8) + align256(4 * N) +
           align256(4 * (N > n_draws ? N : n_draws));
}

inline McmcWs ws_carve(void* ws, long long N, long long n_draws) {
    const long long nb = (N + 255) / 256;
    char* p = (char*)ws;
    McmcWs w;
    w.cdf = (unsigned long long*)p; p += align256(8 * N);
    w.block = (unsigned long long*)p; p += align256(8 * nb);
    w.block_dead = (int*)p; p += align256(4 * nb);
    w.total = (unsigned long long*)p; p += align256(8);
    w.counts = (int*)p; p += align256(4 * N);
    w.src = (int*)p;
    (void)n_draws;
    return w;
}

__global__ void __launch_bounds__(256)
mcmc_weights_kernel(int N, const float* __restrict__ opac, float thresh, unsigned long long* __restrict__ cdf,
                    unsigned long long* __restrict__ block, int* __restrict__ block_dead, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long w = 0ull;
    bool dead = false;
    if (i < N) {
        const float x = opac[i];
        w = draw_weight(x, thresh);
        dead = is_dead(x, thresh);
        cdf[i] = w;
        counts[i] = 0;
    }
    w = (unsigned long long)wave_sum_ll((long long)w);
    const unsigned long long dm = __ballot(dead);
    __shared__ unsigned long long s_w[4];
    __shared__ int s_d[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_w[wave] = w; s_d[wave] = __popcll(dm); }
    __syncthreads();
    if (threadIdx.x == 0) {
        block[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        block_dead[blockIdx.x] = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
    }
}

// one workgroup: exclusive bases of the workgroup sums (in place), the total weight and the dead count
__global__ void __launch_bounds__(1024)
mcmc_scan_blocks_kernel(int nb, unsigned long long* __restrict__ block, const int* __restrict__ block_dead,
                        unsigned long long* __restrict__ total, int* __restrict__ n_dead) {
    __shared__ unsigned long long s_wave[16];
    __shared__ unsigned long long s_base;
    __shared__ int s_dead[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0ull;
    int dead = 0;
    __syncthreads();
    for (int start = 0; start < nb; start += 1024) {
        const int i = start + tid;
        const unsigned long long v = i < nb ? block[i] : 0ull;
        if (i < nb) dead += block_dead[i];
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long wbase = 0ull, tot = 0ull;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned long long t = s_wave[w];
            if (w < wave) wbase += t;
            tot += t;
        }
        if (i < nb) block[i] = s_base + wbase + incl - v;
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    dead = wave_sum_i(dead);
    if (lane == 0) s_dead[wave] = dead;
    __syncthreads();
    if (tid == 0) {
        int d = 0;
        for (int w = 0; w < 16; ++w) d += s_dead[w];
        total[0] = s_base;
        if (n_dead) n_dead[0] = d;
    }
}

__global__ void __launch_bounds__(256)
mcmc_prefix_kernel(int N, unsigned long long* __restrict__ cdf, const unsigned long long* __restrict__ block) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long v = i < N ? cdf[i] : 0ull;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __shared__ unsigned long long s_wave[4];
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (i >= N) return;
    unsigned long long base = block[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    cdf[i] = base + incl;
}

// ---- draws -------------------------------------------------------------------------------------------------------
// relocate: every dead slot draws one live source (or takes the caller's; a source that is out of range or dead itself
// is ignored: the slot then keeps its row)
__global__ void __launch_bounds__(256)
mcmc_relocate_draw_kernel(int N, const float* __restrict__ opac, float min_opacity, const int* __restrict__ sources,
                          const unsigned long long* __restrict__ cdf, const unsigned long long* __restrict__ total,
                          unsigned long long seed, unsigned long long counter, int* __restrict__ slot_src,
                          int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int src = -1;
    if (is_dead(opac[i], min_opacity)) {
        if (sources) {
            src = sources[i];
            if (src < 0 || src >= N || is_dead(opac[src], min_opacity)) src = -1;
        } else {
            const unsigned long long tot = total[0];
            if (tot > 0ull) src = draw_row(cdf, N, tot, rng64(seed, counter, (unsigned long long)i, kRngRelocate));
        }
    }
    slot_src[i] = src;
    if (src >= 0) atomicAdd(&counts[src], 1);
}

// add / sample: n draws over all rows; rows outside [0, N) of the caller's list are clamped (memory safety only).
// With a zero total weight the draw falls back to row k mod N.
__global__ void __launch_bounds__(256)
mcmc_draw_kernel(int N, long long n, const int* __restrict__ sources, const unsigned long long* __restrict__ cdf,
                 const unsigned long long* __restrict__ total, unsigned long long seed, unsigned long long counter,
                 int* __restrict__ out, int* __restrict__ counts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    int src;
    if (sources) {
        src = min(max(sources[k], 0), N - 1);
    } else {
        const unsigned long long tot = total[0];
        src = tot > 0ull ? draw_row(cdf, N, tot, rng64(seed, counter, (unsigned long long)k, kRngSample))
                         : (int)(k % N);
    }
    out[k] = src;
    if (counts) atomicAdd(&counts[src], 1);
}

// ---- the relocation formula of a source drawn c times (ratio = c + 1, clamped to n_max), in fp64 --------------------
//   sigma' = 1 - (1 - sigma)^(1/ratio)  (as -expm1(log1p(-sigma)/ratio)), clamped to [min_opacity, 1 - 2^-23]
//   s'     = s sigma / sum_{j=1..ratio} C(ratio, j) (-1)^(j-1) sigma'^j / sqrt(j)
// (the hockey-stick form of gsplat's double sum sum_{i=1..ratio} sum_{k<i} C(i-1,k) (-1)^k sigma'^(k+1)/sqrt(k+1))
__global__ void __launch_bounds__(256)
mcmc_update_kernel(int N, float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, EmitLayout L,
                   const int* __restrict__ counts, float min_opacity, int zero_moments) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = counts[i];
    if (c == 0) return;
    const int ratio = min(c + 1, kMcmcNMax);
    float* op = params + L.old_begin[3] + i;
    const double sig = 1.0 / (1.0 + exp(-(double)op[0]));
    double sp = -expm1(log1p(-sig) / ratio);
    sp = fmin(fmax(sp, (double)min_opacity), 1.0 - 1.0 / 8388608.0);
    double denom = 0.0, binom = 1.0, pw = 1.0;
    for (int j = 1; j <= ratio; ++j) {
        binom = binom * (double)(ratio - j + 1) / (double)j;         // C(ratio, j): exact below 2^53
        pw *= sp;
        const double t = binom * pw / sqrt((double)j);
        denom += (j & 1) ? t : -t;
    }
    op[0] = (float)log(sp / (1.0 - sp));
    const double lf = log(sig / denom);
    float* sc = params + L.old_begin[1] + (size_t)i * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) sc[k] = (float)((double)sc[k] + lf);
    if (zero_moments) {
        for (int g = 0; g < 6; ++g) {
            const int w = L.width[g];
            const size_t b = (size_t)L.old_begin[g] + (size_t)i * w;
            for (int k = 0; k < w; ++k) { m[b + k] = 0.f; v[b + k] = 0.f; }
        }
    }
}

__device__ __forceinline__ void group_of(const EmitLayout& L, int c, int& g, int& k) {
    g = 0; k = c;
    while (k >= L.width[g]) { k -= L.width[g]; ++g; }
}

// relocate: every group of a dead slot <- its (updated) source; 64 lanes per slot, 4 slots per workgroup
__global__ void __launch_bounds__(256)
mcmc_copy_kernel(int N, const int* __restrict__ slot_src, float* params, EmitLayout L) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int src = slot_src[i];
    if (src < 0) return;
    for (int c = threadIdx.x & 63; c < L.total_width; c += 64) {
        int g, k;
        group_of(L, c, g, k);
        const int w = L.width[g];
        params[(size_t)L.old_begin[g] + (size_t)i * w + k] = params[(size_t)L.old_begin[g] + (size_t)src * w + k];
    }
}

// add: rows [0, N) of the three buffers as they are, then one copy of each drawn source with zero moments
__global__ void __launch_bounds__(256)
mcmc_emit_kernel(int N, int n_add, const int* __restrict__ draws, const float* __restrict__ old_p,
                 const float* __restrict__ old_m, const float* __restrict__ old_v, float* __restrict__ new_p,
                 float* __restrict__ new_m, float* __restrict__ new_v, EmitLayout L) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long long)N + n_add) return;
    const bool appended = r >= N;
    const long long src = appended ? draws[r - N] : r;
    for (int c = threadIdx.x & 63; c < L.total_width; c += 64) {
        int g, k;
        group_of(L, c, g, k);
        const int w = L.width[g];
        const size_t s = (size_t)L.old_begin[g] + (size_t)src * w + k;
        const size_t d = (size_t)L.new_begin[g] + (size_t)r * w + k;
        new_p[d] = old_p[s];
        new_m[d] = appended ? 0.f : old_m[s];
        new_v[d] = appended ? 0.f : old_v[s];
    }
}

// ---- noise ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void box_muller(unsigned long long h, float& z0, float& z1) {
    const float u1 = (float)((h >> 40) + 1ull) * (1.f / 16777216.f);           // (0, 1]
    const float u2 = (float)((h >> 16) & 0xffffffull) * (1.f / 16777216.f);    // [0, 1)
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

struct NoiseArgs {
    float lr, noise_lr;
    const float* dev_lr;          // non-null: the means rate in device memory (replaces lr)
    long long step;
    const float* dev_state;       // non-null: dev_state[0] is the step (replaces step)
    unsigned long long seed;
    const int* skip;
};

__global__ void __launch_bounds__(256)
mcmc_noise_kernel(int N, float* __restrict__ means, const float* __restrict__ scales, const float* __restrict__ quats,
                  const float* __restrict__ opac, const float* __restrict__ noise, NoiseArgs a) {
    if (a.skip != nullptr && a.skip[0] != 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float sig = 1.f / (1.f + expf(-opac[i]));
    const float gate = 1.f / (1.f + expf(-100.f * ((1.f - sig) - 0.995f)));
    const float lr = a.dev_lr ? a.dev_lr[0] : a.lr;
    const float scaler = gate * lr * a.noise_lr;
    float e0, e1, e2;
    if (noise) {
        e0 = noise[(size_t)3 * i]; e1 = noise[(size_t)3 * i + 1]; e2 = noise[(size_t)3 * i + 2];
    } else {
        const unsigned long long step = a.dev_state ? (unsigned long long)(long long)a.dev_state[0]
                                                    : (unsigned long long)a.step;
        float unused;
        box_muller(rng64(a.seed, step, (unsigned long long)i, kRngNoise0), e0, e1);
        box_muller(rng64(a.seed, step, (unsigned long long)i, kRngNoise1), e2, unused);
    }
    float w = quats[(size_t)4 * i], x = quats[(size_t)4 * i + 1], y = quats[(size_t)4 * i + 2],
          z = quats[(size_t)4 * i + 3];
    const float inv = 1.f / sqrtf(w * w + x * x + y * y + z * z);
    w *= inv; x *= inv; y *= inv; z *= inv;
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - w * z), R02 = 2.f * (x * z + w * y);
    const float R10 = 2.f * (x * y + w * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - w * x);
    const float R20 = 2.f * (x * z - w * y), R21 = 2.f * (y * z + w * x), R22 = 1.f - 2.f * (x * x + y * y);
    const float s0 = expf(scales[(size_t)3 * i]), s1 = expf(scales[(size_t)3 * i + 1]), s2 = expf(scales[(size_t)3 * i + 2]);
    e0 *= scaler; e1 *= scaler; e2 *= scaler;
    // Sigma e = R (diag(s^2) (R^T e))
    const float t0 = (R00 * e0 + R10 * e1 + R20 * e2) * (s0 * s0);
    const float t1 = (R01 * e0 + R11 * e1 + R21 * e2) * (s1 * s1);
    const float t2 = (R02 * e0 + R12 * e1 + R22 * e2) * (s2 * s2);
    float* mp = means + (size_t)3 * i;
    mp[0] += R00 * t0 + R01 * t1 + R02 * t2;
    mp[1] += R10 * t0 + R11 * t1 + R12 * t2;
    mp[2] += R20 * t0 + R21 * t1 + R22 * t2;
}

// ---- regularisers ---------------------------------------------------------------------------------------------------
struct RegArgs {
    float co, cs;                 // lambda_o / N, lambda_s / (3 N): gradient coefficients for an upstream gradient of 1
    const float* up_o;            // non-null: device upstream gradient of the opacity term
    const float* up_s;
};

__global__ void __launch_bounds__(256)
mcmc_reg_kernel(int N, const float* __restrict__ scales, const float* __restrict__ opac, RegArgs a,
                float* __restrict__ g_scales, float* __restrict__ g_opac, double* __restrict__ partials) {
    const float co = g_opac ? a.co * (a.up_o ? a.up_o[0] : 1.f) : 0.f;
    const float cs = g_scales ? a.cs * (a.up_s ? a.up_s[0] : 1.f) : 0.f;
    double v[2] = {0.0, 0.0};                                 // sum of opacities, sum of scales
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const float sig = 1.f / (1.f + expf(-opac[i]));
        const float e0 = expf(scales[(size_t)3 * i]), e1 = expf(scales[(size_t)3 * i + 1]),
                    e2 = expf(scales[(size_t)3 * i + 2]);
        v[0] += (double)sig;
        v[1] += (double)e0 + (double)e1 + (double)e2;
        if (g_opac) g_opac[i] += co * (sig * (1.f - sig));
        if (g_scales) {
            float* g = g_scales + (size_t)3 * i;
            g[0] += cs * e0; g[1] += cs * e1; g[2] += cs * e2;
        }
    }
    if (!partials) return;
    __shared__ double s_w[2][4];
    __shared__ double s[2];
    block_sum_d(v, s_w, s);
    if (threadIdx.x < 2) partials[2 * blockIdx.x + threadIdx.x] = s[threadIdx.x];
}

// fixed-order fold of the block partials (one workgroup): out = (reg_o, reg_s, reg_o + reg_s)
__global__ void __launch_bounds__(256)
mcmc_reg_fold_kernel(const double* __restrict__ partials, int nb, double wo, double ws, float* __restrict__ out) {
    double v[2] = {0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += 256) { v[0] += partials[2 * b]; v[1] += partials[2 * b + 1]; }
    __shared__ double s_w[2][4];
    __shared__ double s[2];
    block_sum_d(v, s_w, s);
    if (threadIdx.x == 0) {
        const float ro = (float)(wo * s[0]), rs = (float)(ws * s[1]);
        out[0] = ro; out[1] = rs; out[2] = ro + rs;
    }
}

// the weights and their prefix: ws.cdf / ws.total (and the dead count), counts zeroed
inline void launch_prefix(int N, const float* opac, float thresh, const McmcWs& w, int* n_dead, hipStream_t st) {
    const int nb = (N + 255) / 256;
    hipLaunchKernelGGL(mcmc_weights_kernel, dim3(nb), dim3(256), 0, st, N, opac, thresh, w.cdf, w.block, w.block_dead,
                       w.counts);
    hipLaunchKernelGGL(mcmc_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, nb, w.block, w.block_dead, w.total, n_dead);
    hipLaunchKernelGGL(mcmc_prefix_kernel, dim3(nb), dim3(256), 0, st, N, w.cdf, w.block);
}

}  // namespace qed

using namespace qed;

extern "C" int64_t qed_mcmc_workspace_bytes(int32_t N, int64_t n_draws) {
    if (N < 0 || n_draws < 0) return QED_E_INVALID_ARG;
    return ws_bytes(N, n_draws);
}

extern "C" int qed_mcmc_sample(int32_t N, const float* opacities, float min_opacity, int64_t n_draws, uint64_t seed,
                               uint64_t counter, int32_t* out_idx, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    QED_REQUIRE(N >= 0 && n_draws >= 0, "bad arguments");
    QED_REQUIRE(n_draws == 0 || N >= 1, "draws from an empty set");
    if (n_draws == 0) return QED_OK;
    QED_REQUIRE(n_draws < (1ll << 31) * 256ll, "too many draws");
    QED_REQUIRE(opacities && out_idx && workspace, "null buffers");
    QED_REQUIRE(workspace_bytes >= ws_bytes(N, n_draws), "workspace too small (qed_mcmc_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const McmcWs w = ws_carve(workspace, N, n_draws);
    launch_prefix(N, opacities, min_opacity, w, nullptr, st);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((unsigned)((n_draws + 255) / 256)), dim3(256), 0, st, N, (long long)n_draws,
                       nullptr, w.cdf, w.total, (unsigned long long)seed, (unsigned long long)counter, out_idx, nullptr);
    return check_launch("qed_mcmc_sample");
}

extern "C" int qed_mcmc_relocate(int32_t N, float* params, float* exp_avg, float* exp_avg_sq,
                                 const int64_t* h_group_begin, float min_opacity, const int32_t* sources, uint64_t seed,
                                 uint64_t counter, int32_t* n_dead, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    QED_REQUIRE(N >= 0 && h_group_begin, "bad arguments");
    if (N == 0) return QED_OK;
    QED_REQUIRE(params && exp_avg && exp_avg_sq && workspace, "null buffers");
    QED_REQUIRE(h_group_begin[0] == 0, "group begins must start at 0");
    EmitLayout L;
    const int rc = emit_layout("qed_mcmc_relocate", N, h_group_begin, 0, nullptr, L);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(workspace_bytes >= ws_bytes(N, N), "workspace too small (qed_mcmc_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const McmcWs w = ws_carve(workspace, N, N);
    const float* opac = params + L.old_begin[3];
    const int nb = (N + 255) / 256;
    launch_prefix(N, opac, min_opacity, w, n_dead, st);
    hipLaunchKernelGGL(mcmc_relocate_draw_kernel, dim3(nb), dim3(256), 0, st, N, opac, min_opacity, sources, w.cdf,
                       w.total, (unsigned long long)seed, (unsigned long long)counter, w.src, w.counts);
    hipLaunchKernelGGL(mcmc_update_kernel, dim3(nb), dim3(256), 0, st, N, params, exp_avg, exp_avg_sq, L, w.counts,
                       min_opacity, 1);
    hipLaunchKernelGGL(mcmc_copy_kernel, dim3((N + 3) / 4), dim3(256), 0, st, N, w.src, params, L);
    return check_launch("qed_mcmc_relocate");
}

extern "C" int qed_mcmc_add(int32_t N, int32_t n_add, float* params, const float* exp_avg, const float* exp_avg_sq,
                            const int64_t* h_old_begin, float min_opacity, const int32_t* sources, uint64_t seed,
                            uint64_t counter, float* new_params, float* new_exp_avg, float* new_exp_avg_sq,
                            const int64_t* h_new_begin, void* workspace, int64_t workspace_bytes, void* stream) {
    QED_REQUIRE(N >= 1 && n_add >= 0 && h_old_begin && h_new_begin, "bad arguments");
    QED_REQUIRE((long long)N + n_add < (1ll << 31), "N + n_add too large");
    if (n_add == 0) return QED_OK;
    QED_REQUIRE(params && exp_avg && exp_avg_sq && workspace, "null source buffers");
    QED_REQUIRE(new_params && new_exp_avg && new_exp_avg_sq, "null destination buffers");
    QED_REQUIRE(h_old_begin[0] == 0 && h_new_begin[0] == 0, "group begins must start at 0");
    EmitLayout L;
    const int rc = emit_layout("qed_mcmc_add", N, h_old_begin, (long long)N + n_add, h_new_begin, L);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(workspace_bytes >= ws_bytes(N, n_add), "workspace too small (qed_mcmc_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const McmcWs w = ws_carve(workspace, N, n_add);
    const float* opac = params + L.old_begin[3];
    launch_prefix(N, opac, 0.f, w, nullptr, st);                      // (weights unused when sources are given)
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((n_add + 255) / 256), dim3(256), 0, st, N, (long long)n_add, sources,
                       w.cdf, w.total, (unsigned long long)seed, (unsigned long long)counter, w.src, w.counts);
    hipLaunchKernelGGL(mcmc_update_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, params, (float*)nullptr,
                       (float*)nullptr, L, w.counts, min_opacity, 0);
    const long long rows = (long long)N + n_add;
    hipLaunchKernelGGL(mcmc_emit_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, N, n_add, w.src, params,
                       exp_avg, exp_avg_sq, new_params, new_exp_avg, new_exp_avg_sq, L);
    return check_launch("qed_mcmc_add");
}

extern "C" int qed_mcmc_noise(int32_t N, float* means, const float* scales, const float* quats, const float* opacities,
                              const float* noise, float lr, const float* dev_lr, float noise_lr, int64_t step,
                              const float* dev_state, uint64_t seed, const int32_t* skip_flag, void* stream) {
    QED_REQUIRE(N >= 0 && step >= 0, "bad arguments");
    if (N == 0) return QED_OK;
    QED_REQUIRE(means && scales && quats && opacities, "null buffers");
    NoiseArgs a{lr, noise_lr, dev_lr, (long long)step, dev_state, (unsigned long long)seed, skip_flag};
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, means, scales,
                       quats, opacities, noise, a);
    return check_launch("qed_mcmc_noise");
}

extern "C" int qed_mcmc_reg(int32_t N, const float* scales, const float* opacities, float opacity_reg, float scale_reg,
                            float* out, float* grad_scales, float* grad_opacities, const float* v_opacity_reg,
                            const float* v_scale_reg, double* workspace, void* stream) {
    QED_REQUIRE(N >= 1 && scales && opacities, "bad arguments");
    QED_REQUIRE(!out || workspace, "values need the workspace");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)std::min<long long>(kMcmcRegBlocks, ((long long)N + 255) / 256);
    RegArgs a{(float)((double)opacity_reg / N), (float)((double)scale_reg / (3.0 * N)), v_opacity_reg, v_scale_reg};
    hipLaunchKernelGGL(mcmc_reg_kernel, dim3(nb), dim3(256), 0, st, N, scales, opacities, a, grad_scales, grad_opacities,
                       out ? workspace : nullptr);
    if (out)
        hipLaunchKernelGGL(mcmc_reg_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb,
                           (double)opacity_reg / N, (double)scale_reg / (3.0 * N), out);
    return check_launch("qed_mcmc_reg");
}
