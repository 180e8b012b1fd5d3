// Blending contribution of every Gaussian over a view (qed_contribution) and the keep flags / slots of a prune
// (qed_prune_classify), for gfx950 (wave64).
//
// Contribution: the walk of the compositing forward (composite.hip) without its colour arithmetic and without any
// per-pixel output.  Per (view, pixel) Gaussian i contributes w = alpha T_before where the forward pass applies it; per
// Gaussian the kernel leaves max w, sum w and the number of pixels with w > 0 in three integer buffers that accumulate
// across calls:
//   max_weight  u32   the bit pattern of a non-negative float (an integer max IS the float max)
//   sum_weight  u64   fixed point, 32 fractional bits.  Capacity 2^32 units of weight per Gaussian: one Gaussian would have
//                     to fill every pixel of 2 000 views at 1920x1080 at alpha 0.999 to reach it.  Not guarded.
//   hits        u32
// All three are updated with order-independent integer atomics, so the result has the same bits for any order of views
// and any launch order of tiles.  The partial sum of one (tile, Gaussian) is formed in float in a FIXED lane order and
// converted once, round to nearest.
//
// Shape: one wave per 16x16 tile, four pixels per lane (one per 8x8 quadrant), exact-conservative culling per quadrant by
// ballot, the batch's records parked in LDS and fetched by broadcast reads, the two alpha forms chosen per Gaussian by
// gaussian_is_fast, the conic pre-scaled by -log2(e)/2 -- the device functions of composite.hip RESTATED here (not moved
// to a shared header: the compositing kernels' register allocation is tuned to the statement, see their comments, and
// this file must not be able to move it).  Every accept / skip / terminate decision is the one the render made.
//
// Reduction (the design work): per visited Gaussian every lane holds the sum and the max of its four pixels' weights.
//   * hits is a population count of the accept ballots: scalar side, free.
//   * sum and max: every lane PARKS its two values in LDS (stores issue beside the vector pipe; lane = bank, conflict
//     free); after kPark = 8 Gaussians the wave folds them: lane (s, p) = (lane >> 3, lane & 7) reads the eight partials
//     8 p .. 8 p + 7 of parked Gaussian s (two 16-byte reads per quantity), adds them in a fixed tree, and three DPP steps
//     inside the 8-lane group finish it -- 6 cross-lane instructions per EIGHT Gaussians instead of 12 per Gaussian for
//     an in-wave butterfly (a DPP op costs 4.3 issue cycles against 2.2-2.5 for a plain one: scripts/ubench/xlane_cycles.hip).
//     A Gaussian that no pixel accepted is not parked at all.
//   * the folded values of a batch sit in LDS at the Gaussian's batch position t; at the end of the batch lane t issues
//     the three atomics of Gaussian t if it contributed: one full-width wave instruction per quantity and batch, not one
//     single-lane instruction per Gaussian.
// Measured at config B (500 k Gaussians, 1920x1080; profiles/importance.txt): 212 us per view against 141 for the
// compositing forward on the same lists -- 150 us the bare walk, ~40 the park and fold, ~25 the atomics; the in-wave
// butterfly per Gaussian instead of the park: 274 us.
#include "qed_common.h"

// Development switches (A/B builds: python -m qed_splatter_amd.build --variant NAME -DQED_IMP_REDUCE=1; numbers in
// profiles/importance.txt):
//   QED_IMP_REDUCE    0 = park the lanes' partials in LDS, fold eight Gaussians at a time (the product form),
//                     1 = an in-wave butterfly per Gaussian (DPP inside the rows, two shuffles across them),
//                     2 = no reduction and no flush at all: the bare walk (diagnostic: results are not written)
//   QED_IMP_NOATOMIC  the product form without the three atomics of the flush (diagnostic)
#ifndef QED_IMP_REDUCE
#define QED_IMP_REDUCE 0
#endif

namespace qed {
namespace {

typedef unsigned long long u64;
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f3 __attribute__((ext_vector_type(3)));

constexpr int kBatch = 64;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kConicScale = -0.5f * kLog2e;
constexpr int kRecFloats = 8;       // {x, y, k a, k b | k b, k c, opacity or its log2, -}
constexpr int kPark = 8;            // Gaussians parked per fold

// ---- restated from composite.hip (same operations in the same order: bit-identical alphas) --------------------------
__device__ __forceinline__ float sel(u64 m, float a, float b) {
    float d;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(b), "v"(a), "s"(m));
    return d;
}
__device__ __forceinline__ u64 uniform_u64(u64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ bool quadrant_may_touch(const CullGauss& g, int i, int j) {
    const float xl = g.X0 + (float)(8 * i), xh = xl + 7.f, yl = g.Y0 + (float)(8 * j), yh = yl + 7.f;
    auto vline = [&](float X) { const float bb = g.b * X; return edge_min(g.ha * X * X, bb, -bb * g.ic, g.hc, yl, yh); };
    auto hline = [&](float Y) { const float bb = g.b * Y; return edge_min(g.hc * Y * Y, bb, -bb * g.ia, g.ha, xl, xh); };
    const float m = fminf(fminf(vline(xl), vline(xh)), fminf(hline(yl), hline(yh)));
    const bool inside = (xl <= 0.f) & (xh >= 0.f) & (yl <= 0.f) & (yh >= 0.f);
    return inside | !(m > g.thr);
}
__device__ __forceinline__ f2 conic_times_d(f2 R0, f2 R1, f2 d) {
    return __builtin_elementwise_fma(R0, (f2){d.x, d.x}, R1 * (f2){d.y, d.y});
}
__device__ __forceinline__ f3 load_rec_tail(const float4* __restrict__ splats, size_t g) {
    return *reinterpret_cast<const f3*>(&splats[3 * g + 2]);
}
__device__ __forceinline__ bool gaussian_is_fast(float ca, float cb, float cc, float op) {
    return (op <= 0.998f) & (cb * cb <= 0.998f * (ca * cc));
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
constexpr int kDppSwap1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int kDppSwap2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int kDppHalfMirror = 0x141;   // row_half_mirror: lane i <-> 7 - i of each 8-lane group

struct Park {
    float (*psum)[kBatch];              // [kPark][64] per-lane sums of the parked Gaussians
    float (*pmax)[kBatch];
    float* sum;                         // [64] folded values at the Gaussian's batch position
    float* max;
};

// fold the n parked Gaussians (slot s holds batch position byte s of `slots`): a fixed order for every lane count
__device__ __forceinline__ void fold_parked(const Park& pk, int n, u64 slots, int lane) {
    __syncthreads();                                    // single wave: orders the parked stores before these reads
    const int s = lane >> 3, p = lane & 7;
    const float4 a0 = *reinterpret_cast<const float4*>(&pk.psum[s][8 * p]);
    const float4 a1 = *reinterpret_cast<const float4*>(&pk.psum[s][8 * p + 4]);
    const float4 b0 = *reinterpret_cast<const float4*>(&pk.pmax[s][8 * p]);
    const float4 b1 = *reinterpret_cast<const float4*>(&pk.pmax[s][8 * p + 4]);
    float v = ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w));
    float m = fmaxf(fmaxf(fmaxf(b0.x, b0.y), fmaxf(b0.z, b0.w)), fmaxf(fmaxf(b1.x, b1.y), fmaxf(b1.z, b1.w)));
    v += dpp<kDppSwap1>(v); m = fmaxf(m, dpp<kDppSwap1>(m));
    v += dpp<kDppSwap2>(v); m = fmaxf(m, dpp<kDppSwap2>(m));
    v += dpp<kDppHalfMirror>(v); m = fmaxf(m, dpp<kDppHalfMirror>(m));
    const int t = (int)((slots >> (8 * s)) & 63);
    if (p == 0 && s < n) { pk.sum[t] = v; pk.max[t] = m; }
    __syncthreads();
}

// one pixel of one quadrant against the current Gaussian: composite.hip's fwd_quadrant without the colours
template <bool MIXED>
__device__ __forceinline__ float weight_quadrant(f2 d, f2 R0, f2 R1, float lo, unsigned slow, u64& done, float& T, int& hits) {
    const f2 md = conic_times_d(R0, R1, d);
    float a;
    u64 m_ok;
    if constexpr (MIXED) asm volatile("" : "+s"(slow));
    if (!MIXED || __builtin_expect(slow == 0, 1)) {
        a = __builtin_amdgcn_exp2f(__builtin_fmaf(d.x, md.x, __builtin_fmaf(d.y, md.y, lo)));
        m_ok = __ballot(a >= kAlphaMin) & ~done;
    } else {
        const float p = __builtin_fmaf(d.x, md.x, d.y * md.y);
        a = fminf(kAlphaMax, lo * __builtin_amdgcn_exp2f(p));
        m_ok = __ballot(p <= 0.f) & __ballot(a >= kAlphaMin) & ~done;
    }
    const float at = a * T;
    const float nT = T - at;
    const u64 m_term = m_ok & __ballot(nT <= kTMin);
    done |= m_term;
    const u64 m_acc = m_ok & ~m_term;
    hits += __builtin_popcountll(m_acc);
    const float w = sel(m_acc, at, 0.f);
    T -= w;
    return w;
}

struct WalkState {
    u64 km, mq[4], done[4];
    float T[4];
    int n_park;
    u64 slots;
    int my_hits;                        // lane t: accepted pixels of the batch's Gaussian t
    float my_sum, my_max;               // (QED_IMP_REDUCE 1) lane t: the wave's sum and max of Gaussian t
};

template <bool MIXED>
__device__ __forceinline__ void walk(WalkState& w, f2 p0, u64 m_slow, const float (*s_rec)[kRecFloats], const Park& pk, int lane) {
    while (w.km) {
        const int t = __builtin_ctzll(w.km);
        const u64 bit = 1ull << t;
        w.km &= ~bit;
        const float4 q0 = *reinterpret_cast<const float4*>(&s_rec[t][0]);      // broadcast: every lane the same record
        const float4 q1 = *reinterpret_cast<const float4*>(&s_rec[t][4]);
        const f2 XY = {q0.x, q0.y}, R0 = {q0.z, q0.w}, R1 = {q1.x, q1.y};
        const f2 d0 = XY - p0;
        const unsigned slow = MIXED ? __builtin_amdgcn_readfirstlane((unsigned)(m_slow >> t) & 1u) : 0u;
        float ws = 0.f, wm = 0.f;
        int hits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(w.mq[q] & bit)) continue;             // wave-uniform: this quadrant cannot see Gaussian t
            f2 d = d0;
            if (q & 1) d.x -= 8.f;
            if (q >> 1) d.y -= 8.f;
            const float wq = weight_quadrant<MIXED>(d, R0, R1, q1.z, slow, w.done[q], w.T[q], hits);
            ws += wq;                                   // (a quadrant that is not visited adds an exact zero: culling on
            wm = fmaxf(wm, wq);                         // or off, the lane's sum has the same bits)
            if (w.done[q] == ~0ull) {                   // quadrant finished: drop it from the masks
                w.mq[q] = 0;
                w.km &= w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
            }
        }
        hits = __builtin_amdgcn_readfirstlane(hits);
#if QED_IMP_REDUCE == 1
        if (hits != 0) {
            const float s = wave_sum(ws), m = wave_max(wm);
            w.my_sum = lane == t ? s : w.my_sum;
            w.my_max = lane == t ? m : w.my_max;
            w.my_hits = lane == t ? hits : w.my_hits;
        }
#elif QED_IMP_REDUCE == 2
        asm volatile("" :: "v"(ws), "v"(wm), "s"(hits));
#else
        if (hits != 0) {                                // wave-uniform: park the lanes' partials of a contributing Gaussian
            pk.psum[w.n_park][lane] = ws;
            pk.pmax[w.n_park][lane] = wm;
            w.slots |= (u64)t << (8 * w.n_park);
            w.my_hits = lane == t ? hits : w.my_hits;
            if (++w.n_park == kPark) {
                fold_parked(pk, kPark, w.slots, lane);
                w.n_park = 0;
                w.slots = 0;
            }
        }
#endif
    }
}

__global__ void __launch_bounds__(64)
contribution_kernel(int C, int N, const float4* __restrict__ splats, const int* __restrict__ flatten_ids,
                    const int* __restrict__ offsets, int width, int height, int tile_w, int tile_h,
                    const unsigned char* __restrict__ pixel_mask, unsigned* __restrict__ max_weight,
                    u64* __restrict__ sum_weight, unsigned* __restrict__ hits_out, int keep_all) {
    __shared__ __attribute__((aligned(16))) float s_rec[kBatch][kRecFloats];
    __shared__ __attribute__((aligned(16))) float s_psum[kPark][kBatch];
    __shared__ __attribute__((aligned(16))) float s_pmax[kPark][kBatch];
    __shared__ float s_sum[kBatch], s_max[kBatch];
    const Park pk{s_psum, s_pmax, s_sum, s_max};
    const int n_tiles = tile_w * tile_h;
    const int tile = xcd_remap(blockIdx.x, C * n_tiles);
    const int start = offsets[tile], end = offsets[tile + 1];
    if (end <= start) return;                           // an empty tile reads no list entry (flatten_ids may be NULL)
    const int cam = tile / n_tiles;
    const int t_in = tile - cam * n_tiles;
    const int ty = t_in / tile_w, tx = t_in - ty * tile_w;
    const int lane = threadIdx.x;
    const int lx = lane & 7, ly = lane >> 3;
    const float ox = (float)(tx * QED_TILE), oy = (float)(ty * QED_TILE);
    const int nb = (end - start + kBatch - 1) / kBatch;
    const f2 p0 = {(float)(tx * QED_TILE + lx) + 0.5f, (float)(ty * QED_TILE + ly) + 0.5f};

    WalkState w;
    w.n_park = 0; w.slots = 0; w.my_hits = 0; w.my_sum = 0.f; w.my_max = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = tx * QED_TILE + ((q & 1) << 3) + lx, iy = ty * QED_TILE + ((q >> 1) << 3) + ly;
        bool live = ix < width && iy < height;
        // a masked-out pixel votes in none of the scores: pixels are independent, so it simply starts out finished
        if (live && pixel_mask != nullptr) live = pixel_mask[((size_t)cam * height + iy) * width + ix] != 0;
        w.done[q] = __ballot(!live);
        w.T[q] = 1.f;
    }

    // the two-deep software pipeline of composite.hip's fwd_tile: unconditional loads from clamped indices
    auto id_at = [&](int idx) { return flatten_ids[idx < end ? idx : end - 1]; };
    int rid_c = id_at(start + lane);
    int rid_n = id_at(start + kBatch + lane);
    float4 r0, r1;
    f3 r2;
    {
        const size_t g = (size_t)rid_c;
        r0 = splats[3 * g]; r1 = splats[3 * g + 1]; r2 = load_rec_tail(splats, g);
    }
    bool present = start + lane < end;
    auto all_done = [&]() { return (w.done[0] & w.done[1] & w.done[2] & w.done[3]) == ~0ull; };
    for (int b = 0; b < nb && !all_done(); ++b) {
        // ---- stage this lane's Gaussian: cull per quadrant, pre-scale the conic ----
        const CullGauss cg = cull_setup(r0, r1, r2.z, ox, oy);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool k = present & ((keep_all != 0) | quadrant_may_touch(cg, q & 1, q >> 1));
            const u64 m = __ballot(k);
            w.mq[q] = w.done[q] == ~0ull ? 0ull : uniform_u64(m);
        }
        w.km = w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
        const bool fast = gaussian_is_fast(r0.z, r0.w, r1.x, r1.y);
        const u64 m_slow = uniform_u64(__ballot(!fast));
        if (w.km) {
            const float bh = kConicScale * r0.w;
            *reinterpret_cast<float4*>(&s_rec[lane][0]) = make_float4(r0.x, r0.y, kConicScale * r0.z, bh);
            *reinterpret_cast<float4*>(&s_rec[lane][4]) =
                make_float4(bh, kConicScale * r1.x, fast ? __builtin_amdgcn_logf(r1.y) : r1.y, 0.f);
        }
        __syncthreads();                                // single wave: orders the stores before the reads below
        // the gather of the next batch (its ids arrived a batch ago) and the id load of the one after
        const size_t g_n = (size_t)rid_n;
        const float4 n0 = splats[3 * g_n], n1 = splats[3 * g_n + 1];
        const f3 n2 = load_rec_tail(splats, g_n);
        const int rid_nn = id_at(start + (b + 2) * kBatch + lane);
        if (m_slow == 0) walk<false>(w, p0, m_slow, s_rec, pk, lane);
        else walk<true>(w, p0, m_slow, s_rec, pk, lane);
        // ---- flush: lane t owns the batch's Gaussian t; a Gaussian leaves the wave at most once per tile, and only if
        // it contributed ----
        if (w.n_park != 0) {
            fold_parked(pk, w.n_park, w.slots, lane);
            w.n_park = 0;
            w.slots = 0;
        }
        if (w.my_hits != 0) {
            const int n = rid_c - cam * N;              // records c N + n of every camera land on row n
#if QED_IMP_REDUCE == 1
            const float v_sum = w.my_sum, v_max = w.my_max;
#else
            const float v_sum = s_sum[lane], v_max = s_max[lane];
#endif
#ifndef QED_IMP_NOATOMIC
            if ((unsigned)n < (unsigned)N) {
                atomicMax(&max_weight[n], __float_as_uint(v_max));
                atomicAdd(&sum_weight[n], __float2ull_rn(v_sum * 4294967296.f));
                atomicAdd(&hits_out[n], (unsigned)w.my_hits);
            }
#else
            asm volatile("" :: "v"(v_sum), "v"(v_max), "v"(n));
#endif
            w.my_hits = 0;
        }
        r0 = n0; r1 = n1; r2 = n2;                      // rotate the pipeline
        rid_c = rid_n;
        rid_n = rid_nn;
        present = start + (b + 1) * kBatch + lane < end;
    }
}

// ---- prune: keep flags and the slots of the kept rows (qed_densify_emit's flags / pos) -----------------------------
constexpr int kFlagKeepOld = 4;         // densify.hip: bit 2 = keep the old row

__device__ __forceinline__ bool prune_keeps(int i, const double* __restrict__ score, double min_score, int tie_below) {
    const double s = score[i];
    return s > min_score || (s == min_score && i < tie_below);          // (NaN: never kept)
}

// scan step 1: decisions + per-workgroup counts
__global__ void __launch_bounds__(256)
prune_flags_kernel(int N, const double* __restrict__ score, double min_score, int tie_below,
                   unsigned char* __restrict__ flags, int* __restrict__ block_counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < N && prune_keeps(i, score, min_score, tie_below);
    if (i < N) flags[i] = keep ? kFlagKeepOld : 0;
    __shared__ int s_cnt[4];
    const u64 m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// scan step 2: one workgroup turns the per-workgroup counts into exclusive bases (in place) and the total
__global__ void __launch_bounds__(1024)
prune_scan_blocks_kernel(int n_blocks, int* __restrict__ block_counts, int* __restrict__ totals) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int start = 0; start < n_blocks; start += 1024) {
        const int i = start + tid;
        const int v = i < n_blocks ? block_counts[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int t = s_wave[k];
            if (k < wave) wbase += t;
            tot += t;
        }
        if (i < n_blocks) block_counts[i] = s_base + wbase + incl - v;
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) { totals[0] = 0; totals[1] = s_base; totals[2] = 0; totals[3] = 0; }
}

// scan step 3: slot of row i among the kept rows, in qed_densify_emit's column 1
__global__ void __launch_bounds__(256)
prune_positions_kernel(int N, const unsigned char* __restrict__ flags, const int* __restrict__ block_base,
                       int* __restrict__ pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < N && flags[i] != 0;
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (i >= N) return;
    int base = block_base[blockIdx.x];
    for (int k = 0; k < wave; ++k) base += s_cnt[k];
    pos[i] = 0;
    pos[(size_t)N + i] = base + __popcll(m & ((1ull << lane) - 1ull));
    pos[(size_t)2 * N + i] = 0;
    pos[(size_t)3 * N + i] = 0;
}

}  // namespace
}  // namespace qed

using namespace qed;

extern "C" int qed_contribution(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids,
                                const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                const uint8_t* pixel_mask, uint32_t* max_weight, uint64_t* sum_weight, uint32_t* hits,
                                int32_t launch_flags, void* stream) {
    QED_REQUIRE(C >= 1 && N >= 0 && width > 0 && height > 0, "bad extents");
    QED_REQUIRE(tile_w == (width + QED_TILE - 1) / QED_TILE && tile_h == (height + QED_TILE - 1) / QED_TILE,
                "tile grid does not match the image (tile size is 16)");
    QED_REQUIRE(offsets && max_weight && sum_weight && hits, "null buffers");
    QED_REQUIRE(N == 0 || splats, "null splat buffer");
    const long long grid = (long long)C * tile_w * tile_h;
    QED_REQUIRE(grid < (1ll << 29), "too many tiles");
    // flatten_ids may be NULL when the sorted list is empty (offsets are then all zero): nothing to score
    if (N == 0 || flatten_ids == nullptr) return QED_OK;
    hipLaunchKernelGGL(contribution_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, C, N,
                       (const float4*)splats, flatten_ids, offsets, width, height, tile_w, tile_h, pixel_mask, max_weight,
                       (unsigned long long*)sum_weight, hits, (launch_flags & QED_CL_NO_CULL) ? 1 : 0);
    return check_launch("qed_contribution");
}

extern "C" int qed_prune_classify(int32_t N, const double* score, double min_score, int32_t tie_below, uint8_t* flags,
                                  int32_t* pos, int32_t* totals, void* stream) {
    QED_REQUIRE(N >= 1 && score && flags && pos && totals, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (N + 255) / 256;
    int* block_counts = pos + (size_t)4 * N;                 // scratch behind the four position columns
    hipLaunchKernelGGL(prune_flags_kernel, dim3(nb), dim3(256), 0, st, N, score, min_score, tie_below, flags, block_counts);
    hipLaunchKernelGGL(prune_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, nb, block_counts, totals);
    hipLaunchKernelGGL(prune_positions_kernel, dim3(nb), dim3(256), 0, st, N, flags, block_counts, pos);
    return check_launch("qed_prune_classify");
}
