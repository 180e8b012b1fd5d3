// K-channel label fields on frozen Gaussians (qed_features_fwd / qed_features_bwd) and the label kernels that go with
// them (qed_label_loss / qed_label_confusion / qed_label_present), for gfx950 (wave64).  include/qed_splat.h has the
// contract.
//
// The two walking kernels are the walk of the compositing forward (composite.hip) as importance.hip restates it -- one
// wave per 16x16 tile, four pixels per lane (one per 8x8 quadrant), exact-conservative culling per quadrant by ballot, the
// batch's records parked in LDS and fetched by broadcast reads, the two alpha forms chosen per Gaussian -- with the
// device functions RESTATED once more (not moved to a shared header: the compositing kernels' register allocation is
// tuned to their statement and this file must not be able to move it).  Every accept / skip / terminate decision is the
// one the render made, so the weights w = alpha T are the render's own bits.
//
// Channels: a launch is a grid of (tile, channel chunk); a chunk is KC = 4, 8 or 16 channels (the smallest that holds K,
// 16 for K > 8) and every chunk walks its tile's list again.  4 pixels x KC accumulators (forward) or 4 x KC gradient
// values (backward) stay in registers, at most 64; K = 32 with four pixels per lane would be 128.  A (pixel, channel) sum
// runs in list order whatever the chunk, so the chunking cannot be seen in the result.
//   forward   lane t of a batch stages row n_t's chunk next to its record; per visited Gaussian the walk reads the chunk by
//             broadcast and does KC fmas per quadrant that accepted it.
//   backward  per visited Gaussian a lane forms g_k = sum over its four pixels of w v_out[k]; the lanes PARK their KC
//             values in LDS and after kSlots = 4 Gaussians the wave folds them: the 16 lanes of DPP row s own slot s, lane
//             p of the row adds lanes 4 p .. 4 p + 3 in a fixed tree and four DPP steps finish the row -- importance.hip's
//             park and fold, KC values wide.  The folded rows wait in LDS at the Gaussian's batch position; at the end of
//             the batch the wave issues the adds, 64 / KC Gaussians x KC channels per instruction, so that a row's KC floats
//             are one contiguous request (64 lanes in 64 rows is the shape global float atomics are ~17x slower at, and it
//             cost 0.3 of the 1.0 ms at K = 16): one float add per (tile, contributing Gaussian, channel).
//             A Gaussian that no pixel of the tile accepted is neither parked nor added.
// The matrix-instruction forms (v_mfma_f32_32x32x2_f32 on [256 pixels x 64 Gaussians] x [64 x K]) have not been built;
// profiles/semantic.txt says what was measured.
#include "qed_common.h"

// Development switch (A/B builds: python -m qed_splatter_amd.build --variant NAME -DQED_SEM_BWD_MAX_CHUNK=8; numbers in
// profiles/semantic.txt):
//   QED_SEM_BWD_MAX_CHUNK  the widest channel chunk of the backward: 16 (a chunk like the forward's: 27 KB of LDS per wave at
//                          K > 8) or 8 (16 KB, one more walk per eight channels)
//   QED_SEM_BWD_FLUSH      0 = an atomic wave instruction covers 64 / KC Gaussians x KC channels: KC contiguous floats per
//                          row (the product form), 1 = lane t adds the KC channels of Gaussian t one after the other: 64
//                          lanes in 64 rows per instruction, the shape global float atomics are ~17x slower at
#ifndef QED_SEM_BWD_MAX_CHUNK
#define QED_SEM_BWD_MAX_CHUNK 16
#endif
#ifndef QED_SEM_BWD_FLUSH
#define QED_SEM_BWD_FLUSH 0
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
constexpr int kSlots = 4;           // Gaussians parked per fold of the backward: one per DPP row
constexpr int kParkPad = 4;         // floats behind a lane's KC parked values: 16-byte stores of 16 lanes hit 64 banks

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
constexpr int kDppRowMirror = 0x140;    // row_mirror: lane i <-> 15 - i of each 16-lane row

// one pixel of one quadrant against the current Gaussian: composite.hip's fwd_quadrant without the colours.  Returns the
// weight the forward pass applies (0 where it does not); n_acc = the number of pixels of the quadrant that accepted it
template <bool MIXED>
__device__ __forceinline__ float weight_quadrant(f2 d, f2 R0, f2 R1, float lo, unsigned slow, u64& done, float& T, int& n_acc) {
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
    n_acc = __builtin_popcountll(m_acc);
    const float w = sel(m_acc, at, 0.f);
    T -= w;
    return w;
}

struct WalkState {
    u64 km, mq[4], done[4];
    float T[4];
};

// the part of a tile's walk both kernels share: the ids, the two-deep record pipeline, cull and stage.  `Body` supplies what
// differs: stage(lane's row n, staged?) before the barrier, prefetch(next row n) behind it, walk(m_slow) and flush(row n).
struct TileGeom {
    int start, end, cam, tx, ty;
};

__device__ __forceinline__ bool tile_geom(TileGeom& g, int C, const int* __restrict__ offsets, int tile_w, int tile_h) {
    const int n_tiles = tile_w * tile_h;
    const int tile = xcd_remap(blockIdx.x, C * n_tiles);
    g.start = offsets[tile];
    g.end = offsets[tile + 1];
    g.cam = tile / n_tiles;
    const int t_in = tile - g.cam * n_tiles;
    g.ty = t_in / tile_w;
    g.tx = t_in - g.ty * tile_w;
    return g.end > g.start;
}

// row n's channels k0 .. k0 + KC - 1 (zeros past K and for a row outside the table)
template <int KC>
__device__ __forceinline__ void load_row_chunk(float (&f)[KC], const float* __restrict__ table, int n, int N, int K, int k0) {
#pragma unroll
    for (int k = 0; k < KC; ++k) f[k] = 0.f;
    if ((unsigned)n >= (unsigned)N) return;
    const float* row = table + (size_t)n * K + k0;
    if ((K & 3) == 0) {                                 // rows and chunks start on 16 bytes: whole float4 groups
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            if (k0 + 4 * j < K) {
                const float4 v = *reinterpret_cast<const float4*>(row + 4 * j);
                f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) if (k0 + k < K) f[k] = row[k];
    }
}

// ================================================================================================
// forward
// ================================================================================================
template <int KC, bool MIXED>
__device__ __forceinline__ void walk_fwd(WalkState& w, f2 p0, u64 m_slow, const float (*s_rec)[kRecFloats],
                                         const float (*s_feat)[KC], float (&acc)[4][KC]) {
    while (w.km) {
        const int t = __builtin_ctzll(w.km);
        const u64 bit = 1ull << t;
        w.km &= ~bit;
        const float4 q0 = *reinterpret_cast<const float4*>(&s_rec[t][0]);      // broadcast: every lane the same record
        const float4 q1 = *reinterpret_cast<const float4*>(&s_rec[t][4]);
        float f[KC];
#pragma unroll
        for (int j = 0; j < KC / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(&s_feat[t][4 * j]);
            f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
        }
        const f2 XY = {q0.x, q0.y}, R0 = {q0.z, q0.w}, R1 = {q1.x, q1.y};
        const f2 d0 = XY - p0;
        const unsigned slow = MIXED ? __builtin_amdgcn_readfirstlane((unsigned)(m_slow >> t) & 1u) : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(w.mq[q] & bit)) continue;             // wave-uniform: this quadrant cannot see Gaussian t
            f2 d = d0;
            if (q & 1) d.x -= 8.f;
            if (q >> 1) d.y -= 8.f;
            int n_acc;
            const float wq = weight_quadrant<MIXED>(d, R0, R1, q1.z, slow, w.done[q], w.T[q], n_acc);
            // (a lane that did not accept adds w f = an exact zero: culling on or off, visited or skipped, the same bits --
            // for a FINITE table, which the contract asks for: 0 * inf is NaN)
            if (n_acc != 0) {
#pragma unroll
                for (int k = 0; k < KC; ++k) acc[q][k] = __builtin_fmaf(wq, f[k], acc[q][k]);
            }
            if (w.done[q] == ~0ull) {                   // quadrant finished: drop it from the masks
                w.mq[q] = 0;
                w.km &= w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
            }
        }
    }
}

template <int KC>
__global__ void __launch_bounds__(64)
features_fwd_kernel(int C, int N, int K, const float4* __restrict__ splats, const int* __restrict__ flatten_ids,
                    const int* __restrict__ offsets, int width, int height, int tile_w, int tile_h,
                    const float* __restrict__ features, float* __restrict__ out, int keep_all) {
    __shared__ __attribute__((aligned(16))) float s_rec[kBatch][kRecFloats];
    __shared__ __attribute__((aligned(16))) float s_feat[kBatch][KC];
    TileGeom tg;
    const bool any = tile_geom(tg, C, offsets, tile_w, tile_h);
    const int k0 = blockIdx.y * KC;
    const int lane = threadIdx.x;
    const int lx = lane & 7, ly = lane >> 3;
    float acc[4][KC];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[q][k] = 0.f;

    if (any) {                                          // an empty tile reads no list entry (and writes its zeros below)
        const int start = tg.start, end = tg.end, cam = tg.cam;
        const float ox = (float)(tg.tx * QED_TILE), oy = (float)(tg.ty * QED_TILE);
        const int nb = (end - start + kBatch - 1) / kBatch;
        const f2 p0 = {(float)(tg.tx * QED_TILE + lx) + 0.5f, (float)(tg.ty * QED_TILE + ly) + 0.5f};
        WalkState w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ix = tg.tx * QED_TILE + ((q & 1) << 3) + lx, iy = tg.ty * QED_TILE + ((q >> 1) << 3) + ly;
            w.done[q] = __ballot(!(ix < width && iy < height));
            w.T[q] = 1.f;
        }
        // the two-deep software pipeline of composite.hip's fwd_tile: unconditional loads from clamped indices
        auto id_at = [&](int idx) { return flatten_ids[idx < end ? idx : end - 1]; };
        int rid_c = id_at(start + lane);
        int rid_n = id_at(start + kBatch + lane);
        float4 r0, r1;
        f3 r2;
        float fr[KC];
        {
            const size_t g = (size_t)rid_c;
            r0 = splats[3 * g]; r1 = splats[3 * g + 1]; r2 = load_rec_tail(splats, g);
            load_row_chunk<KC>(fr, features, rid_c - cam * N, N, K, k0);    // records c N + n of every camera read row n
        }
        bool present = start + lane < end;
        auto all_done = [&]() { return (w.done[0] & w.done[1] & w.done[2] & w.done[3]) == ~0ull; };
        for (int b = 0; b < nb && !all_done(); ++b) {
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
#pragma unroll
                for (int j = 0; j < KC / 4; ++j)
                    *reinterpret_cast<float4*>(&s_feat[lane][4 * j]) =
                        make_float4(fr[4 * j], fr[4 * j + 1], fr[4 * j + 2], fr[4 * j + 3]);
            }
            __syncthreads();                            // single wave: orders the stores before the reads below
            // the gather of the next batch (its ids arrived a batch ago) and the id load of the one after
            const size_t g_n = (size_t)rid_n;
            const float4 n0 = splats[3 * g_n], n1 = splats[3 * g_n + 1];
            const f3 n2 = load_rec_tail(splats, g_n);
            float fn[KC];
            load_row_chunk<KC>(fn, features, rid_n - cam * N, N, K, k0);
            const int rid_nn = id_at(start + (b + 2) * kBatch + lane);
            if (m_slow == 0) walk_fwd<KC, false>(w, p0, m_slow, s_rec, s_feat, acc);
            else walk_fwd<KC, true>(w, p0, m_slow, s_rec, s_feat, acc);
            __syncthreads();                            // the walk's reads before the next batch's stores
            r0 = n0; r1 = n1; r2 = n2;                  // rotate the pipeline
#pragma unroll
            for (int k = 0; k < KC; ++k) fr[k] = fn[k];
            rid_c = rid_n;
            rid_n = rid_nn;
            present = start + (b + 1) * kBatch + lane < end;
        }
    }

    // every in-image pixel is written (zeros where nothing contributed), nothing outside the image
    const bool vec = (K & 3) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = tg.tx * QED_TILE + ((q & 1) << 3) + lx, iy = tg.ty * QED_TILE + ((q >> 1) << 3) + ly;
        if (!(ix < width && iy < height)) continue;
        float* o = out + (((size_t)tg.cam * height + iy) * width + ix) * K + k0;
        if (vec) {
#pragma unroll
            for (int j = 0; j < KC / 4; ++j)
                if (k0 + 4 * j < K)
                    *reinterpret_cast<float4*>(o + 4 * j) =
                        make_float4(acc[q][4 * j], acc[q][4 * j + 1], acc[q][4 * j + 2], acc[q][4 * j + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < KC; ++k) if (k0 + k < K) o[k] = acc[q][k];
        }
    }
}

// ================================================================================================
// backward
// ================================================================================================
template <int KC>
struct Park {
    float (*lanes)[kBatch][KC + kParkPad];  // [kSlots][64][KC (+ pad)] the lanes' values of the parked Gaussians
    float (*rows)[KC + 1];                  // [64][KC (+ 1: lane = bank)] folded rows at the Gaussian's batch position
};

// fold the n parked Gaussians (slot s holds batch position byte s of `slots`): a fixed order for every lane count
template <int KC>
__device__ __forceinline__ void fold_parked(const Park<KC>& pk, int n, unsigned slots, int lane) {
    __syncthreads();                                    // single wave: orders the parked stores before these reads
    const int s = lane >> 4, p = lane & 15;
    float v[KC];
#pragma unroll
    for (int j = 0; j < KC / 4; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(&pk.lanes[s][4 * p][4 * j]);
        const float4 b = *reinterpret_cast<const float4*>(&pk.lanes[s][4 * p + 1][4 * j]);
        const float4 c = *reinterpret_cast<const float4*>(&pk.lanes[s][4 * p + 2][4 * j]);
        const float4 d = *reinterpret_cast<const float4*>(&pk.lanes[s][4 * p + 3][4 * j]);
        v[4 * j] = (a.x + b.x) + (c.x + d.x);
        v[4 * j + 1] = (a.y + b.y) + (c.y + d.y);
        v[4 * j + 2] = (a.z + b.z) + (c.z + d.z);
        v[4 * j + 3] = (a.w + b.w) + (c.w + d.w);
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        v[k] += dpp<kDppSwap1>(v[k]);
        v[k] += dpp<kDppSwap2>(v[k]);
        v[k] += dpp<kDppHalfMirror>(v[k]);
        v[k] += dpp<kDppRowMirror>(v[k]);
    }
    const int t = (int)((slots >> (8 * s)) & 63u);
    if (p == 0 && s < n) {
#pragma unroll
        for (int k = 0; k < KC; ++k) pk.rows[t][k] = v[k];
    }
    __syncthreads();
}

struct BwdState {
    int n_park;
    unsigned slots;
    int my_hit;                         // lane t: the batch's Gaussian t contributed to a pixel of the tile
};

template <int KC, bool MIXED>
__device__ __forceinline__ void walk_bwd(WalkState& w, BwdState& s, f2 p0, u64 m_slow, const float (*s_rec)[kRecFloats],
                                         const Park<KC>& pk, const float (&vo)[4][KC], int lane) {
    while (w.km) {
        const int t = __builtin_ctzll(w.km);
        const u64 bit = 1ull << t;
        w.km &= ~bit;
        const float4 q0 = *reinterpret_cast<const float4*>(&s_rec[t][0]);
        const float4 q1 = *reinterpret_cast<const float4*>(&s_rec[t][4]);
        const f2 XY = {q0.x, q0.y}, R0 = {q0.z, q0.w}, R1 = {q1.x, q1.y};
        const f2 d0 = XY - p0;
        const unsigned slow = MIXED ? __builtin_amdgcn_readfirstlane((unsigned)(m_slow >> t) & 1u) : 0u;
        float g[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) g[k] = 0.f;
        int hits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(w.mq[q] & bit)) continue;
            f2 d = d0;
            if (q & 1) d.x -= 8.f;
            if (q >> 1) d.y -= 8.f;
            int n_acc;
            const float wq = weight_quadrant<MIXED>(d, R0, R1, q1.z, slow, w.done[q], w.T[q], n_acc);
            if (n_acc != 0) {
#pragma unroll
                for (int k = 0; k < KC; ++k) g[k] = __builtin_fmaf(wq, vo[q][k], g[k]);
            }
            hits += n_acc;
            if (w.done[q] == ~0ull) {
                w.mq[q] = 0;
                w.km &= w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
            }
        }
        hits = __builtin_amdgcn_readfirstlane(hits);
        if (hits != 0) {                                // wave-uniform: park the lanes' values of a contributing Gaussian
#pragma unroll
            for (int j = 0; j < KC / 4; ++j)
                *reinterpret_cast<float4*>(&pk.lanes[s.n_park][lane][4 * j]) =
                    make_float4(g[4 * j], g[4 * j + 1], g[4 * j + 2], g[4 * j + 3]);
            s.slots |= (unsigned)t << (8 * s.n_park);
            s.my_hit = lane == t ? 1 : s.my_hit;
            if (++s.n_park == kSlots) {
                fold_parked<KC>(pk, kSlots, s.slots, lane);
                s.n_park = 0;
                s.slots = 0;
            }
        }
    }
}

template <int KC>
__global__ void __launch_bounds__(64)
features_bwd_kernel(int C, int N, int K, const float4* __restrict__ splats, const int* __restrict__ flatten_ids,
                    const int* __restrict__ offsets, int width, int height, int tile_w, int tile_h,
                    const float* __restrict__ v_out, float* __restrict__ v_features, int keep_all) {
    __shared__ __attribute__((aligned(16))) float s_rec[kBatch][kRecFloats];
    __shared__ __attribute__((aligned(16))) float s_lanes[kSlots][kBatch][KC + kParkPad];
    __shared__ float s_rows[kBatch][KC + 1];
    __shared__ int s_row_of[kBatch];                    // the table row of the batch's Gaussian t, -1: nothing to add
    const Park<KC> pk{s_lanes, s_rows};
    TileGeom tg;
    if (!tile_geom(tg, C, offsets, tile_w, tile_h)) return;     // an empty tile reads no list entry
    const int start = tg.start, end = tg.end, cam = tg.cam;
    const int k0 = blockIdx.y * KC;
    const int lane = threadIdx.x;
    const int lx = lane & 7, ly = lane >> 3;
    const float ox = (float)(tg.tx * QED_TILE), oy = (float)(tg.ty * QED_TILE);
    const int nb = (end - start + kBatch - 1) / kBatch;
    const f2 p0 = {(float)(tg.tx * QED_TILE + lx) + 0.5f, (float)(tg.ty * QED_TILE + ly) + 0.5f};

    WalkState w;
    BwdState s;
    s.n_park = 0; s.slots = 0; s.my_hit = 0;
    float vo[4][KC];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = tg.tx * QED_TILE + ((q & 1) << 3) + lx, iy = tg.ty * QED_TILE + ((q >> 1) << 3) + ly;
        const bool live = ix < width && iy < height;
        w.done[q] = __ballot(!live);
        w.T[q] = 1.f;
        // a pixel's chunk of v_out is one row of a [C H W, K] table
        load_row_chunk<KC>(vo[q], v_out, live ? (int)(((size_t)cam * height + iy) * width + ix) : -1, C * height * width, K, k0);
    }

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
        const size_t g_n = (size_t)rid_n;
        const float4 n0 = splats[3 * g_n], n1 = splats[3 * g_n + 1];
        const f3 n2 = load_rec_tail(splats, g_n);
        const int rid_nn = id_at(start + (b + 2) * kBatch + lane);
        if (m_slow == 0) walk_bwd<KC, false>(w, s, p0, m_slow, s_rec, pk, vo, lane);
        else walk_bwd<KC, true>(w, s, p0, m_slow, s_rec, pk, vo, lane);
        // ---- flush: lane t owns the batch's Gaussian t; a Gaussian leaves the wave at most once per tile, and only if
        // it contributed ----
        if (s.n_park != 0) {
            fold_parked<KC>(pk, s.n_park, s.slots, lane);
            s.n_park = 0;
            s.slots = 0;
        }
#if QED_SEM_BWD_FLUSH == 1
        if (s.my_hit != 0) {
            const int n = rid_c - cam * N;              // records c N + n of every camera land on row n
            if ((unsigned)n < (unsigned)N) {
                float* row = v_features + (size_t)n * K + k0;
#pragma unroll
                for (int k = 0; k < KC; ++k) if (k0 + k < K) atomicAdd(row + k, s_rows[lane][k]);
            }
            s.my_hit = 0;
        }
#else
        // lane t publishes the row of its Gaussian; then instruction j adds Gaussians j G .. j G + G - 1 (G = 64 / KC), lane
        // l channel l % KC of Gaussian j G + l / KC: KC contiguous floats per row and request, not 64 rows per instruction
        {
            const int n = rid_c - cam * N;              // records c N + n of every camera land on row n
            const bool add = s.my_hit != 0 && (unsigned)n < (unsigned)N;
            s_row_of[lane] = add ? n : -1;
            const u64 any = __ballot(add);
            s.my_hit = 0;
            __syncthreads();                            // single wave: orders the stores before the reads below
            if (any != 0) {
                constexpr int G = kBatch / KC;
                const int k = lane % KC, sub = lane / KC;
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    if (((any >> (j * G)) & ((1ull << G) - 1ull)) == 0) continue;       // wave-uniform: none of these G
                    const int t = j * G + sub;
                    const int row = s_row_of[t];
                    if (row >= 0 && k0 + k < K) atomicAdd(v_features + (size_t)row * K + k0 + k, s_rows[t][k]);
                }
            }
        }
#endif
        __syncthreads();                                // the flush's reads before the next batch's stores
        r0 = n0; r1 = n1; r2 = n2;                      // rotate the pipeline
        rid_c = rid_n;
        rid_n = rid_nn;
        present = start + (b + 1) * kBatch + lane < end;
    }
}

// ================================================================================================
// the label kernels
// ================================================================================================
constexpr int kLossGrid = QED_LABEL_LOSS_WS_DOUBLES / 2 - 1;        // workgroups of the reduce pass (256)

// a labelled pixel: its label is a class of the table and not the ignore value
__device__ __forceinline__ bool labelled(int y, int K, int ignore_label) { return y != ignore_label && y < K; }

// log-sum-exp of a row about its maximum: mx and the sum of exp(x - mx)
__device__ __forceinline__ void row_lse(const float* __restrict__ x, int K, float& mx, float& se) {
    mx = x[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
    se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(x[k] - mx);
}

// pass 1: per workgroup the sum of w_y nll and the sum of w_y over the labelled pixels, as doubles
__global__ void __launch_bounds__(256)
label_loss_reduce_kernel(long long n_pix, int K, const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                         int ignore_label, const float* __restrict__ class_weight, double* __restrict__ ws) {
    __shared__ double s_w[2][4], s[2];
    double v[2] = {0.0, 0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256) {
        const int y = labels[i];
        if (!labelled(y, K, ignore_label)) continue;
        const float* x = logits + (size_t)i * K;
        float mx, se;
        row_lse(x, K, mx, se);
        const double nll = (double)(mx - x[y]) + (double)logf(se);
        const double cw = class_weight != nullptr ? (double)class_weight[y] : 1.0;
        v[0] += cw * nll;
        v[1] += cw;
    }
    block_sum_d<2, 256>(v, s_w, s);
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = s[0]; ws[2 * blockIdx.x + 1] = s[1]; }
}

// pass 2: every workgroup folds the n_part partials in the same fixed order (thread t owns partial t), then writes the
// gradient rows of its pixels; workgroup 0 also writes the loss and the two totals
__global__ void __launch_bounds__(256)
label_loss_finish_kernel(long long n_pix, int K, const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                         int ignore_label, const float* __restrict__ class_weight, int n_part, double* __restrict__ ws,
                         float* __restrict__ v_logits, float* __restrict__ loss) {
    __shared__ double s_w[2][4], s[2];
    double p[2] = {0.0, 0.0};
    if ((int)threadIdx.x < n_part) { p[0] = ws[2 * threadIdx.x]; p[1] = ws[2 * threadIdx.x + 1]; }
    block_sum_d<2, 256>(p, s_w, s);
    const double sum = s[0], wsum = s[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ws[2 * kLossGrid] = sum;
        ws[2 * kLossGrid + 1] = wsum;
        loss[0] = wsum > 0.0 ? (float)(sum / wsum) : 0.f;
    }
    if (v_logits == nullptr) return;
    const float inv = wsum > 0.0 ? (float)(1.0 / wsum) : 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256) {
        const int y = labels[i];
        float* g = v_logits + (size_t)i * K;
        if (!labelled(y, K, ignore_label) || inv == 0.f) {
            for (int k = 0; k < K; ++k) g[k] = 0.f;
            continue;
        }
        const float* x = logits + (size_t)i * K;
        float mx, se;
        row_lse(x, K, mx, se);
        const float scale = (class_weight != nullptr ? class_weight[y] : 1.f) * inv;
        const float rs = 1.f / se;
        for (int k = 0; k < K; ++k) g[k] = scale * (expf(x[k] - mx) * rs - (k == y ? 1.f : 0.f));
    }
}

// the first maximum of a row (ties go to the lower index; a NaN never wins)
__device__ __forceinline__ int row_argmax(const float* __restrict__ x, int K) {
    int best = 0;
    float mx = x[0];
    for (int k = 1; k < K; ++k) {
        const float v = x[k];
        if (v > mx || (mx != mx && v == v)) { mx = v; best = k; }
    }
    return best;
}

// a histogram per workgroup in LDS, then one 64-bit integer add per non-zero cell
__global__ void __launch_bounds__(256)
label_confusion_kernel(long long n_pix, int K, const float* __restrict__ logits, const unsigned char* __restrict__ labels,
                       int ignore_label, const float* __restrict__ acc, float min_alpha, u64* __restrict__ confusion) {
    __shared__ unsigned s_hist[QED_FEATURES_MAX * (QED_FEATURES_MAX + 1)];
    const int cells = K * (K + 1);
    for (int c = threadIdx.x; c < cells; c += 256) s_hist[c] = 0u;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256) {
        const int y = labels[i];
        if (!labelled(y, K, ignore_label)) continue;
        int pred = row_argmax(logits + (size_t)i * K, K);
        if (acc != nullptr && !(acc[i] >= min_alpha)) pred = K;
        atomicAdd(&s_hist[y * (K + 1) + pred], 1u);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {
        const unsigned v = s_hist[c];
        if (v != 0u) atomicAdd(&confusion[c], (u64)v);
    }
}

__global__ void __launch_bounds__(256)
label_present_kernel(long long n_pix, int K, const float* __restrict__ logits, const float* __restrict__ acc, float min_alpha,
                     const unsigned char* __restrict__ palette, unsigned char* __restrict__ out_label,
                     unsigned char* __restrict__ out_rgb) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256) {
        int pred = row_argmax(logits + (size_t)i * K, K);
        const bool none = acc != nullptr && !(acc[i] >= min_alpha);
        if (none) pred = K;
        if (out_label != nullptr) out_label[i] = none ? (unsigned char)QED_LABEL_NONE : (unsigned char)pred;
        if (out_rgb != nullptr) {
            out_rgb[3 * i] = palette[3 * pred];
            out_rgb[3 * i + 1] = palette[3 * pred + 1];
            out_rgb[3 * i + 2] = palette[3 * pred + 2];
        }
    }
}

int check_walk_args(const char* who, int C, int N, int K, int width, int height, int tile_w, int tile_h) {
    if (!(C >= 1 && N >= 0 && width > 0 && height > 0)) {
        set_error("%s: bad extents", who);
        return QED_E_INVALID_ARG;
    }
    if (!(K >= 1 && K <= QED_FEATURES_MAX)) {
        set_error("%s: the channel count must be in 1..%d", who, QED_FEATURES_MAX);
        return QED_E_INVALID_ARG;
    }
    if (!(tile_w == (width + QED_TILE - 1) / QED_TILE && tile_h == (height + QED_TILE - 1) / QED_TILE)) {
        set_error("%s: tile grid does not match the image (tile size is 16)", who);
        return QED_E_INVALID_ARG;
    }
    if ((long long)C * tile_w * tile_h >= (1ll << 29) || (long long)C * N >= (1ll << 31) ||
        (long long)C * width * height >= (1ll << 31)) {
        set_error("%s: too many tiles, records or pixels", who);
        return QED_E_INVALID_ARG;
    }
    return QED_OK;
}

// the channel chunk of a launch: the smallest of 4, 8, 16 that holds K, 16 beyond
inline int chunk_of(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : 16; }
inline int chunk_of_bwd(int K) { const int kc = chunk_of(K); return kc < QED_SEM_BWD_MAX_CHUNK ? kc : QED_SEM_BWD_MAX_CHUNK; }

int check_label_args(const char* who, long long n_pix, int K, const void* logits, const void* labels) {
    if (!(n_pix >= 0 && K >= 1 && K <= QED_FEATURES_MAX)) {
        set_error("%s: bad extents (the class count must be in 1..%d)", who, QED_FEATURES_MAX);
        return QED_E_INVALID_ARG;
    }
    if (n_pix > 0 && !(logits && labels)) {
        set_error("%s: null buffers", who);
        return QED_E_INVALID_ARG;
    }
    return QED_OK;
}

}  // namespace
}  // namespace qed

using namespace qed;

extern "C" int qed_features_fwd(int32_t C, int32_t N, int32_t K, const float* splats, const int32_t* flatten_ids,
                                const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                const float* features, float* out, int32_t launch_flags, void* stream) {
    const int rc = check_walk_args("qed_features_fwd", C, N, K, width, height, tile_w, tile_h);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(offsets && out, "null buffers");
    QED_REQUIRE(N == 0 || (splats && features), "null splat or feature buffer");
    QED_REQUIRE(((uintptr_t)features & 15) == 0 && ((uintptr_t)out & 15) == 0, "features and out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0 || flatten_ids == nullptr) {
        // no record or an empty sorted list (offsets are then all zero): nothing was composited
        (void)hipMemsetAsync(out, 0, sizeof(float) * (size_t)C * width * height * K, st);
        return check_launch("qed_features_fwd");
    }
    const int kc = chunk_of(K);
    const dim3 grid((unsigned)((long long)C * tile_w * tile_h), (unsigned)((K + kc - 1) / kc));
    const int keep_all = (launch_flags & QED_CL_NO_CULL) ? 1 : 0;
#define QED_LAUNCH_FWD(KC)                                                                                              \
    hipLaunchKernelGGL(features_fwd_kernel<KC>, grid, dim3(64), 0, st, C, N, K, (const float4*)splats, flatten_ids, offsets, \
                       width, height, tile_w, tile_h, features, out, keep_all)
    if (kc == 4) QED_LAUNCH_FWD(4);
    else if (kc == 8) QED_LAUNCH_FWD(8);
    else QED_LAUNCH_FWD(16);
#undef QED_LAUNCH_FWD
    return check_launch("qed_features_fwd");
}

extern "C" int qed_features_bwd(int32_t C, int32_t N, int32_t K, const float* splats, const int32_t* flatten_ids,
                                const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                const float* v_out, float* v_features, int32_t launch_flags, void* stream) {
    const int rc = check_walk_args("qed_features_bwd", C, N, K, width, height, tile_w, tile_h);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(offsets && v_out, "null buffers");
    QED_REQUIRE(((uintptr_t)v_out & 15) == 0, "v_out must be 16-byte aligned");
    if (N == 0 || flatten_ids == nullptr) return QED_OK;         // nothing was composited: no gradient
    QED_REQUIRE(splats && v_features, "null splat or gradient buffer");
    const int kc = chunk_of_bwd(K);
    const dim3 grid((unsigned)((long long)C * tile_w * tile_h), (unsigned)((K + kc - 1) / kc));
    const int keep_all = (launch_flags & QED_CL_NO_CULL) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
#define QED_LAUNCH_BWD(KC)                                                                                              \
    hipLaunchKernelGGL(features_bwd_kernel<KC>, grid, dim3(64), 0, st, C, N, K, (const float4*)splats, flatten_ids, offsets, \
                       width, height, tile_w, tile_h, v_out, v_features, keep_all)
    if (kc == 4) QED_LAUNCH_BWD(4);
    else if (kc == 8) QED_LAUNCH_BWD(8);
    else QED_LAUNCH_BWD(16);
#undef QED_LAUNCH_BWD
    return check_launch("qed_features_bwd");
}

extern "C" int qed_label_loss(int64_t n_pix, int32_t K, const float* logits, const uint8_t* labels, int32_t ignore_label,
                              const float* class_weight, double* workspace, float* v_logits, float* loss, void* stream) {
    const int rc = check_label_args("qed_label_loss", n_pix, K, logits, labels);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(workspace && loss, "null buffers");
    hipStream_t st = (hipStream_t)stream;
    const unsigned g1 = stream_grid(n_pix, kLossGrid);
    hipLaunchKernelGGL(label_loss_reduce_kernel, dim3(g1), dim3(256), 0, st, (long long)n_pix, K, logits, labels, ignore_label,
                       class_weight, workspace);
    const unsigned g2 = v_logits != nullptr ? stream_grid(n_pix) : 1u;
    hipLaunchKernelGGL(label_loss_finish_kernel, dim3(g2), dim3(256), 0, st, (long long)n_pix, K, logits, labels, ignore_label,
                       class_weight, (int)g1, workspace, v_logits, loss);
    return check_launch("qed_label_loss");
}

extern "C" int qed_label_confusion(int64_t n_pix, int32_t K, const float* logits, const uint8_t* labels, int32_t ignore_label,
                                   const float* acc, float min_alpha, uint64_t* confusion, void* stream) {
    const int rc = check_label_args("qed_label_confusion", n_pix, K, logits, labels);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(confusion, "null buffers");
    QED_REQUIRE(acc == nullptr || min_alpha == min_alpha, "min_alpha is NaN");
    if (n_pix == 0) return QED_OK;
    hipLaunchKernelGGL(label_confusion_kernel, dim3(stream_grid(n_pix, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (long long)n_pix, K, logits, labels, ignore_label, acc, min_alpha, (unsigned long long*)confusion);
    return check_launch("qed_label_confusion");
}

extern "C" int qed_label_present(int64_t n_pix, int32_t K, const float* logits, const float* acc, float min_alpha,
                                 const uint8_t* palette, uint8_t* out_label, uint8_t* out_rgb, void* stream) {
    QED_REQUIRE(n_pix >= 0 && K >= 1 && K <= QED_FEATURES_MAX, "bad extents");
    QED_REQUIRE(out_label || out_rgb, "no output plane");
    QED_REQUIRE(out_rgb == nullptr || palette, "the colour plane needs a palette");
    QED_REQUIRE(acc == nullptr || min_alpha == min_alpha, "min_alpha is NaN");
    if (n_pix == 0) return QED_OK;
    QED_REQUIRE(logits, "null logits");
    hipLaunchKernelGGL(label_present_kernel, dim3(stream_grid(n_pix)), dim3(256), 0, (hipStream_t)stream, (long long)n_pix, K,
                       logits, acc, min_alpha, palette, out_label, out_rgb);
    return check_launch("qed_label_present");
}
